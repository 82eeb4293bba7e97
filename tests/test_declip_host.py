"""CPU: the declipper's reference (tests/declip_reference.py) alone - that the restatement restores what it should, that float64 is
enough, and that the GPU tests' batches (tests/declip_cases.py) hold what those tests say they hold - and the host side of
data.Declipper: the header, the signatures, the argument checks."""
import ctypes

import numpy as np
import pytest
import torch

import declip_cases as C
import declip_reference as D
import screen_reference as SR
from isp_tts_amd import runtime
from isp_tts_amd.data import Declipper

LEVELS = (0.7, 0.5, 0.3)


@pytest.fixture(scope="module")
def restored():
    """level -> (clean, clipped, float64 result, longdouble result) on clip(22050, 4096)."""
    x = D.clip(22050, 4096)
    out = {}
    for level in LEVELS:
        y = D.hard_clip(x, level)
        out[level] = (x, y, D.declip_item(y, 4096, 4096), D.declip_item(y, 4096, 4096, dtype=np.longdouble))
    return out


def test_the_reference_restores(restored):
    for level in LEVELS:
        x, y, r, _ = restored[level]
        m = r["mask"]
        before, after = D.sdr_db(x, y, m), D.sdr_db(x, r["audio"], m)
        print(f"clip level {level}: {int(m.sum())} unknown samples, SDR over them {before:.1f} dB -> {after:.1f} dB")
        assert r["dense"] == 0 and r["windows"] > 0 and r["restored"] == r["clip_samples"] == int(m.sum()), level
        assert r["flags"] == D.FLAGS["restored"]
        if level == 0.5:
            assert after - before >= 15.0
        # consistent with the clipping: never inside the rail, and nothing else moved
        got, was = r["audio"][:4096], y
        assert (np.abs(got[m]) >= np.abs(was[m])).all() and (np.sign(got[m]) == np.sign(was[m])).all()
        assert np.array_equal(got[~m].view(np.int32), was[~m].view(np.int32))
        assert r["peak"] == np.abs(got).max()


def test_float64_is_enough(restored):
    for level in LEVELS:
        _, _, r, rl = restored[level]
        m = r["mask"]
        u = D.ulps(r["audio"][:4096][m], rl["audio"][:4096][m])
        print(f"clip level {level}: {100.0 * (u > 0).mean():.3f} % of the restored samples differ from the longdouble run, at most {u.max()} ulp")
        assert u.max() <= 1 and (u > 0).mean() <= 0.01
        assert all(r[k] == rl[k] for k in ("clip_samples", "restored", "windows", "dense", "flags"))


def test_the_mask_is_the_screens_counted_runs(restored):
    for level in LEVELS:
        _, y, r, _ = restored[level]
        for min_run in (1, 3, 7):
            s = SR.screen_item(y, 4096, 4096, min_run=min_run)
            want = np.zeros(4096, bool)
            for start, length, _ in s["rail_runs"]:
                if length >= min_run:
                    want[start:start + length] = True
            got = D.declip_item(y, 4096, 4096, min_run=min_run, iterations=1, order=4)
            assert np.array_equal(got["mask"], want) and got["clip_samples"] == s["clip_samples"] and got["thr"] == s["thr"]


def test_a_clipped_sinusoid_is_dense():
    y = C.sinusoid()
    r = D.declip_item(y, C.S, C.S)
    m = r["mask"]
    assert all(m[max(0, 512 * j - 256):512 * j + 768].sum() > D.MAX_UNKNOWNS and m[512 * j:512 * j + 512].any() for j in range(8))
    assert r["dense"] == 8 and r["windows"] == 0 and r["restored"] == 0 and r["flags"] == D.FLAGS["dense"]
    assert np.array_equal(r["audio"].view(np.int32), y.view(np.int32))


def test_the_gpu_batch_holds_its_cases():
    c = C.batch()
    items, ref = C.reference()
    m0, y0 = items[0]["mask"], c["audio"][0]
    runs = {(s, n): cls for s, n, cls in SR.runs_of(np.where(y0 >= items[0]["thr"], 1, np.where(y0 <= -items[0]["thr"], 2, 0)))}
    for name, (b, start, length, sign) in c["planted"].items():
        inside = items[b]["mask"][start:start + length]
        if name in ("below_min_run",):
            assert not inside.any() and (start, length) in runs                 # a run of its own, one sample short
        elif name == "run63":
            assert inside.all() and (start, length) in runs
        elif b == 0 and name in ("min_run", "plus", "minus", "run64", "split"):
            assert inside.all() and runs[(start, length)] == (1 if sign > 0 else 2), name
        else:
            assert inside.all(), name
    assert m0[0] and m0[C.LENS[0] - 1] and items[1]["mask"][C.LENS[1] - 1]
    assert m0[511] and m0[512] and m0[767] and m0[768] and m0[1023] and m0[1024] and not m0[1022]
    p, q = c["planted"]["plus"], c["planted"]["minus"]
    assert q[1] == p[1] + p[2]
    assert ref["dense"].tolist() == [0, 0, 0] and ref["windows"].tolist()[2] == 1 and 4 <= ref["restored"].tolist()[2] <= 6
    assert (ref["flags"] == D.FLAGS["restored"]).all()
    # the configurations reach what they are for
    assert C.reference("mr64")[1]["clip_samples"].tolist() == [64, 0, 0] and C.reference("mr64")[1]["restored"].tolist() == [64, 0, 0]
    assert (C.reference("mr1")[1]["clip_samples"] - ref["clip_samples"]).tolist() == [C.MIN_RUN - 1, 0, 1]      # the short run; a lone peak
    assert C.reference("rail")[1]["thr"].tolist() == [np.float32(0.44)] * 3
    for name in C.CONFIGS:
        got = C.reference(name)[1]
        assert got["restored"][0] > 0, name
        print(name, {k: got[k].tolist() for k in ("clip_samples", "restored", "windows", "dense", "flags")})


@pytest.mark.parametrize("config", list(C.CONFIGS))
def test_float64_is_enough_on_the_gpu_batch(config):
    """What makes one fp32 ulp and 1 % the right bounds for the device: float64 and the extended run agree that well."""
    items, _ = C.reference(config)
    wide, _ = C.reference(config, "longdouble")
    for b in range(3):
        k = items[b]["kept"]
        assert np.array_equal(k, wide[b]["kept"])
        if k.any():
            u = D.ulps(items[b]["audio"][:len(k)][k], wide[b]["audio"][:len(k)][k])
            assert u.max() <= 1 and (u > 0).mean() <= 0.01, (config, b, u.max(), (u > 0).mean())


def test_the_dense_limit_batch():
    d = C.dense_limit()
    masks = [it["mask"] for it in d["items"]]
    assert [int(m[:768].sum()) for m in masks] == [256, 257, 259] and [int(m[256:].sum()) for m in masks] == [256, 257, 256]
    assert d["ref"]["windows"].tolist() == [2, 0, 1] and d["ref"]["dense"].tolist() == [0, 2, 1]
    assert d["ref"]["restored"].tolist() == [256, 0, 128] and d["ref"]["clip_samples"].tolist() == [256, 257, 259]
    assert d["ref"]["flags"].tolist() == [1, 2, 3]
    wide = [D.declip_item(d["audio"][b], 1024, 1024, dtype=np.longdouble) for b in range(3)]
    for it, w in zip(d["items"], wide):
        k = it["kept"]
        if k.any():
            u = D.ulps(it["audio"][k], w["audio"][k])
            assert u.max() <= 1 and (u > 0).mean() <= 0.01


# ------------------------------------------------------------------------------------------------ the host side
def test_header_and_signatures():
    P, I32, I64, F32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    assert runtime.SIGNATURES["ispk_declip_f64"] == [P, I64, P, P, I32, F32, F32, I32, I32, I32, P, I64] + [P] * 9 + [I64, I32, I32, P]
    assert runtime.SIGNATURES["ispk_declip_workspace_bytes"] == [I32, I32, P] and runtime.SIGNATURES["ispk_declip_max_unknowns"] == []
    lib = runtime.lib()
    assert lib.ispk_declip_max_unknowns() == runtime.DECLIP_MAX_UNKNOWNS == D.MAX_UNKNOWNS
    assert runtime.DECLIP_FLAGS == D.FLAGS and runtime.DECLIP_SEGMENT_SAMPLES == D.H
    for B, S in ((0, 0), (1, 1), (3, 512), (3, 513), (2, 4096), (5, 4097), (7, 131072), (1, 1 << 24)):
        n = ctypes.c_int64(-1)
        assert lib.ispk_declip_workspace_bytes(B, S, ctypes.byref(n)) == 0 and n.value == runtime.declip_workspace_bytes(B, S), (B, S)
    assert [name for name, _, _ in runtime.DECLIP_OUTPUTS] == ["audio_len", "thr", "peak", "clip_samples", "restored", "windows", "dense", "flags"]


def test_refusals_without_a_gpu():
    lib = runtime.lib()
    one = ctypes.c_void_p(1 << 20)                          # never dereferenced: every check fails before a launch
    far = ctypes.c_void_p(1 << 30)
    B, S = 2, 1024
    args = dict(audio=one, ld_audio=S, audio_len=one, in_flags=None, rail_mode=0, rail=0.0, rail_ratio=0.999, min_run=3, order=32,
                iterations=3, out=far, ld_out=S, out_len=one, thr=one, peak=one, clip_samples=one, restored=one, windows=one, dense=one,
                flags=one, workspace=one, workspace_bytes=runtime.declip_workspace_bytes(B, S), B=B, S=S, stream=None)
    E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3
    refused = [(dict(B=65536), E_SHAPE), (dict(S=-1), E_SHAPE), (dict(S=(1 << 24) + 1), E_SHAPE), (dict(rail_mode=2), E_SHAPE),
               (dict(rail_ratio=0.0), E_SHAPE), (dict(rail_ratio=1.5), E_SHAPE), (dict(rail_mode=1, rail=0.0), E_SHAPE),
               (dict(rail_mode=1, rail=float("inf")), E_SHAPE), (dict(min_run=0), E_SHAPE), (dict(min_run=65), E_SHAPE),
               (dict(order=0), E_SHAPE), (dict(order=33), E_SHAPE), (dict(iterations=0), E_SHAPE), (dict(iterations=9), E_SHAPE),
               (dict(ld_audio=S - 1), E_SHAPE), (dict(ld_out=S - 1), E_SHAPE), (dict(out=one), E_SHAPE),
               (dict(out=ctypes.c_void_p((1 << 20) + 4 * S)), E_SHAPE),         # the second row of audio
               (dict(workspace_bytes=runtime.declip_workspace_bytes(B, S) - 1), E_ALIGN),
               (dict(workspace=ctypes.c_void_p((1 << 20) + 4)), E_ALIGN)]
    refused += [({k: None}, E_NULL) for k in ("audio", "audio_len", "out", "out_len", "thr", "peak", "clip_samples", "restored", "windows",
                                              "dense", "flags", "workspace")]
    for kw, code in refused:
        assert lib.ispk_declip_f64(*{**args, **kw}.values()) == code, kw
    assert lib.ispk_declip_f64(*{**args, "B": 0}.values()) == 0                 # a no-op


def test_arguments():
    for kw in (dict(rail="min"), dict(rail=0.0), dict(rail=float("inf")), dict(rail_ratio=0.0), dict(rail_ratio=1.01), dict(min_run=0),
               dict(min_run=65), dict(min_run=2.5), dict(order=0), dict(order=33), dict(iterations=0), dict(iterations=9)):
        with pytest.raises(ValueError):
            Declipper(**kw)
    dc = Declipper()
    assert (dc.rail, dc.rail_ratio, dc.min_run, dc.order, dc.iterations) == ("max", 0.999, 3, 32, 3)
    with pytest.raises(runtime.IspkError, match="GPU tensors"):
        dc(torch.zeros(2, 64), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="audio"):
        dc(torch.zeros(2, 64, dtype=torch.float64), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="audio_len"):
        dc(torch.zeros(2, 64), torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="flags"):
        dc(torch.zeros(2, 64), torch.zeros(2, dtype=torch.int64), flags=torch.zeros(2, dtype=torch.int64))
    out = dc.empty_outputs(3, "cpu", samples=1000)
    assert out["audio"].shape == (3, 1000) and out["work"].numel() == runtime.declip_workspace_bytes(3, 1000)
    assert set(out) == {"audio", "work"} | {name for name, _, _ in runtime.DECLIP_OUTPUTS}
    rows = dc.manifest(dict(audio=None, audio_len=torch.tensor([5, 0]), thr=torch.tensor([0.5, 0.0]), peak=torch.tensor([0.75, 0.0]),
                            clip_samples=torch.tensor([9, 0]), restored=torch.tensor([6, 0]), windows=torch.tensor([1, 0]),
                            dense=torch.tensor([1, 0]), flags=torch.tensor([3, 4])), ["a", "b"])
    assert rows[0] == dict(name="a", audio_len=5, thr=0.5, peak=0.75, clip_samples=9, restored=6, windows=1, dense=1, flags=("restored", "dense"))
    assert rows[1]["flags"] == ("skipped",)
    with pytest.raises(ValueError, match="names"):
        dc.manifest(dict(audio=None, **{k: torch.zeros(2) for k in ("audio_len", "thr", "peak", "clip_samples", "restored", "windows", "dense")},
                         flags=torch.zeros(2, dtype=torch.int32)), ["a"])
