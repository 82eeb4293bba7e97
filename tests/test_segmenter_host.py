"""CPU: the segmenter's host side - the reference's own properties on generated recordings, the margin that makes the GPU
tests' integer comparisons sound, the constructor's conversions and validation, the manifest, the argument checks of the two entry
points (which run before any launch) and the Python face."""
import ctypes

import numpy as np
import pytest
import torch

import segmenter_cases as C
import segmenter_reference as R
from isp_tts_amd import data, runtime
from isp_tts_amd.data import Segmenter

E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3


# ------------------------------------------------------------------------------------------------ the reference's properties
def _recording(g):
    """Noise bursts of random level and pauses (zeros or faint noise) of random length, not aligned to anything."""
    parts = []
    for _ in range(int(g.integers(1, 12))):
        n = int(g.integers(1, 9000))
        parts.append(g.uniform(0.05, 0.5) * g.standard_normal(n))
        m = int(g.integers(0, 6000))
        parts.append(np.zeros(m) if g.random() < 0.5 else 1e-4 * g.standard_normal(m))
    if g.random() < 0.5:
        parts = parts[::-1]
    return np.concatenate(parts).astype(np.float32)


@pytest.mark.parametrize("seed", range(24))
def test_reference_properties(seed):
    g = np.random.default_rng([7, seed])
    x = _recording(g)
    n = len(x)
    pad, msf = int(g.integers(0, 12)), int(g.integers(4, 12))
    max_samples = int(g.integers(1, 30000))
    target, min_samples = int(g.integers(0, max_samples + 1)), int(g.integers(0, 4000))
    ref = "max" if seed % 2 else 0.01
    it = R.plan_item(x, n, n, 1e-4, ref, pad, msf, target, max_samples, min_samples)
    seg, active = it["segments"], it["active"]
    if not active.any():
        assert seg == [] and it["visits"] == []
        return
    assert len(seg) >= 1 and seg[0][0] == it["first"] and seg[-1][1] == it["last"]
    assert 0 <= it["first"] and it["last"] <= n
    for k, (s, e) in enumerate(seg):
        assert s < e, (k, s, e)                                                 # no empty piece
        if k:
            assert seg[k - 1][1] <= s                                           # increasing and disjoint
        assert bool(it["flags"][k] & R.OVER) == (e - s > max_samples) and bool(it["flags"][k] & R.SHORT) == (e - s < min_samples)
    for t in np.flatnonzero(active):                                            # nothing active is cut away
        assert any(s <= R.HOP * t < e for s, e in seg), t
    assert len(it["visits"]) == len(it["candidates"]) + 1 and max(it["visits"]) <= 2 and min(it["visits"]) >= 1
    for (e, s), (e2, _) in zip(it["candidates"], it["candidates"][1:] + [(it["last"], None)]):
        assert e <= s < e2
    for (fr, sp, p_s, p_n), (s, e) in zip(it["levels"], seg):
        assert 0 <= sp <= fr and fr == sum(1 for t in range(len(active)) if s <= R.HOP * t < e)
        assert (p_s > it["thr"] or sp == 0) and p_n <= it["thr"]


def test_cases_hit_every_branch():
    """What each recording of the GPU tests is there for, read off the reference."""
    c = C.small()
    items, plan = C.reference("small", "max")
    it = dict(zip(C.NAMES, items))
    H = C.H
    for name in ("len0", "negative", "beyond", "silent"):
        assert it[name]["segments"] == [], name
    for n in (1, 255, 256, 257, 1023, 1024, 1025):
        assert it[f"len{n}"]["segments"] == [(0, n)], n
    assert it["noise_only"]["segments"] == [(0, 32 * H)]                        # relative to its own max: all active
    assert C.reference("small", "const")[0][C.NAMES.index("noise_only")]["segments"] == []
    assert len(it["no_pause"]["candidates"]) == 0 and len(it["gap_below"]["candidates"]) == 0
    assert it["gap_exact"]["candidates"] == [(14 * H, 15 * H)] and len(it["gap_noise"]["candidates"]) == 1
    wide = dict(zip(C.NAMES, C.reference("small", "wide")[0]))
    assert wide["gap_exact"]["candidates"] == [(14 * H, 14 * H)]                # pad above half the pause: both sides clamp to M
    assert it["lead"]["first"] == 8 * H and len(it["lead"]["candidates"]) == 1
    assert it["trail"]["last"] == 43 * H and len(it["trail"]["candidates"]) == 1
    assert it["over_no_pause"]["flags"] == [R.OVER]
    assert it["look_again"]["visits"] == [1, 2, 1] and it["look_again"]["segments"][0] == (0, 24 * H)
    assert it["look_again"]["flags"][1] == R.OVER
    assert it["at_target"]["segments"][0] == (0, 32 * H) and len(it["below_target"]["segments"]) == 1
    assert it["at_max"]["segments"][0] == (0, 80 * H) and it["at_max"]["flags"][0] == 0 and it["at_max"]["visits"][1] == 1
    assert it["above_max"]["segments"][0] == (0, 24 * H) and it["above_max"]["visits"][1] == 2
    assert it["short_tail"]["flags"][-1] == R.SHORT
    assert len(it["many"]["segments"]) == 13 and plan["wanted"][C.NAMES.index("many")] == 13 > C.K_SMALL == plan["count"][C.NAMES.index("many")]
    assert len(it["ragged"]["segments"]) >= 2
    assert c["S"] % 4 and c["audio"].shape == (len(C.NAMES), c["S"])
    lo = C.long()
    li, lp = C.reference("long", "max")
    assert len(li[0]["p"]) > 8192 and 100 < lp["wanted"][0] <= C.K_LONG and lo["S"] > 2_200_000
    cand, ends = li[0]["candidates"], {e for _, e in li[0]["segments"]}
    assert len(cand) > 256 and cand[127][0] not in ends and cand[128][0] in ends       # a pause passed over at a tile's last slot
    assert sum(e // C.H > 8192 for e, _ in cand) > 8                            # pauses behind the first chunk of 8,192 frames


def test_margin():
    """Every item the GPU tests use keeps its frame powers away from the threshold: min_t |p_t - thr| / thr >= 2^-30 (or thr is 0).
    The kernel's hop sums differ from the exact ones by at most 262 * 2^-53 relative, a frame power by that again and the max by
    the same: a million times less than the margin, so no summation order can flip a decision.  (The smallest margin here is 0.49.)"""
    worst = np.inf
    for batch in ("small", "long"):
        c = C.small() if batch == "small" else C.long()
        for cfg in C.CONFIGS.values():
            for b, (x, n) in enumerate(zip(c["clean"], c["lens"])):
                m, thr = R.margin(x, R.kept_len(n, c["S"]), C.FACTOR, cfg["ref"])
                assert thr == 0.0 or m >= 2.0 ** -30, (batch, cfg, b, m, thr)
                worst = min(worst, m)
    print(f"smallest margin {worst:.3g}")


# ------------------------------------------------------------------------------------------------ the constructor
def test_conversions():
    s = Segmenter(22050)
    assert (s.top_db, s.ref, s.max_segments, s.drop, s.drop_mask) == (40.0, "max", 256, ("over", "short"), 3)
    assert s.factor == 10.0 ** (-40.0 / 10.0)
    assert s.min_silence_frames == (6615 - 1024) // 256 + 1 == 22              # P = round(300 ms) = 6615
    assert s.pad_frames == round(1102.5 / 256) == 4
    assert (s.target_samples, s.max_samples, s.min_samples) == (132300, 441000, 22050)
    t = Segmenter(8000, top_db=30.0, ref=0.5, min_silence_ms=100.0, pad_ms=0.0, target_s=1.0, max_s=2.5, min_s=0.0, max_segments=4096,
                  drop=())
    assert t.min_silence_frames == 4 and t.pad_frames == 0 and t.drop_mask == 0 and t.ref == 0.5     # (800 - 1024) / 256 + 1 floors to 0
    assert (t.target_samples, t.max_samples, t.min_samples) == (8000, 20000, 0)
    assert Segmenter(8000, min_silence_ms=255.9).min_silence_frames == 4 and Segmenter(8000, min_silence_ms=256.0).min_silence_frames == 5
    assert Segmenter(8000, drop="over").drop_mask == 1 and Segmenter(8000, drop=("short",)).drop_mask == 2
    e = s.empty_outputs(3, 5, 64, "cpu", recording_samples=1000)
    assert e["segments"].shape == (3, 256, 2) and e["audio"].shape == (5, 64) and e["rows"].shape == (1,)
    assert e["work"].numel() == runtime.segment_workspace_bytes(3, 1000) == 8 * 3 * (2 * 4 + 2 * 1)
    assert "work" not in s.empty_outputs(3, 5, None, "meta") and s.empty_outputs(1, 2, None, "meta")["audio"].shape == (2, 441000)


def test_validation():
    for kw, match in ((dict(sample_rate=0), "sample_rate"), (dict(sample_rate=22050.5), "sample_rate"), (dict(top_db=0.0), "top_db"),
                      (dict(top_db=float("nan")), "top_db"), (dict(ref="mean"), "ref"), (dict(ref=0.0), "ref"),
                      (dict(min_silence_ms=-1.0), "min_silence_ms"), (dict(pad_ms=-1.0), "pad_ms"), (dict(pad_ms=1e9), "pad_ms"),
                      (dict(target_s=-1.0), "target_s"), (dict(max_s=0.0), "max_s"), (dict(min_s=7.0), "min_s <= target_s"),
                      (dict(target_s=21.0), "min_s <= target_s"), (dict(max_s=1e7), "max_s"), (dict(max_segments=0), "max_segments"),
                      (dict(max_segments=4097), "max_segments"), (dict(max_segments=2.5), "max_segments"),
                      (dict(drop=("long",)), "drop")):
        with pytest.raises(ValueError, match=match):
            Segmenter(**{"sample_rate": 22050, **kw})
    s = Segmenter(8000)
    a, n = torch.zeros((2, 64)), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(runtime.IspkError, match="GPU tensors"):
        s(a, n, rows=4)
    with pytest.raises(runtime.IspkError, match="GPU tensors"):
        s.plan(a, n)
    with pytest.raises(runtime.IspkError, match="GPU tensors"):
        runtime.segment_plan(a, n, 1e-4, 0, 0.0, 1, 4, 100, 200, 10, 8)
    with pytest.raises(ValueError, match="audio"):
        s(a.double(), n, rows=4)
    with pytest.raises(ValueError, match="audio"):
        s(a[:, ::2], n, rows=4)
    with pytest.raises(ValueError, match="audio_len"):
        s(a, n.int(), rows=4)
    with pytest.raises(ValueError, match="audio_len"):
        s(a, n[:1], rows=4)
    with pytest.raises(ValueError, match="rows"):
        s(a, n)
    with pytest.raises(ValueError, match="rows"):
        s(a, n, rows=65536)
    with pytest.raises(ValueError, match="samples"):
        s(a, n, rows=4, samples=-1)
    s.min_silence_frames = 3
    with pytest.raises(ValueError, match="min_silence_frames"):
        s._checked(_Cuda(a), _Cuda(n))
    s.min_silence_frames, s.pad_frames = 4, 65537
    with pytest.raises(ValueError, match="pad_frames"):
        s._checked(_Cuda(a), _Cuda(n))
    s.pad_frames, s.max_samples = 0, 0
    with pytest.raises(ValueError, match="max_samples"):
        s._checked(_Cuda(a), _Cuda(n))


class _Cuda:
    """A CPU tensor that says it is on the GPU: lets the attribute checks behind the device check run without one."""

    def __init__(self, t):
        self._t = t

    def __getattr__(self, name):
        return True if name == "is_cuda" else getattr(self._t, name)


# ------------------------------------------------------------------------------------------------ the manifest
def test_manifest():
    s = Segmenter(8000)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)                          # noqa: E731
    r = dict(rows=i32([3]), item=i32([0, 0, 2, -1]), index=i32([0, 1, 0, 0]), row_flags=i32([0, 2, 5, 0]),
             bounds=torch.tensor([[0, 8000], [9000, 9400], [256, 40256], [0, 0]], dtype=torch.int64))
    assert s.manifest(r, ["a", "b", "c"]) == [("a", 0, 0.0, 1.0, ()), ("a", 1, 1.125, 1.175, ("short",)),
                                              ("c", 0, 0.032, 5.032, ("over", "cut"))]
    assert s.manifest(r, ["a", "b", "c"], sample_rate=16000)[0] == ("a", 0, 0.0, 0.5, ())
    with pytest.raises(ValueError, match="names"):
        s.manifest(r, ["a", "b"])
    with pytest.raises(ValueError, match="sample_rate"):
        s.manifest(r, ["a", "b", "c"], sample_rate=0)
    r["rows"] = i32([0])
    assert s.manifest(r, []) == []


# ------------------------------------------------------------------------------------------------ the C entry points
def _plan_args(**kw):
    one = ctypes.c_void_p(1 << 20)                                              # never dereferenced: the checks come before any launch
    a = dict(audio=one, ld_audio=8192, audio_len=one, factor=1e-4, ref_mode=0, ref=0.0, pad=1, min_silence_frames=4, target_samples=100,
             max_samples=200, min_samples=10, segments=one, flags=one, count=one, wanted=one, frames=one, speech_frames=one,
             speech_power=one, noise_power=one, workspace=one, workspace_bytes=runtime.segment_workspace_bytes(2, 8192), B=2, S=8192, K=8,
             stream=None)
    a.update(kw)
    return list(a.values())


def _gather_args(**kw):
    one, two = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 24)
    a = dict(audio=one, ld_audio=8192, segments=one, flags=one, count=one, drop=3, out=two, ld_out=64, out_len=one, item=one, index=one,
             bounds=one, row_flags=one, rows=one, rows_wanted=one, B=2, S=8192, K=8, R=4, S_out=64, stream=None)
    a.update(kw)
    return list(a.values())


PLAN_REFUSALS = [(dict(B=65536), E_SHAPE), (dict(B=-1), E_SHAPE), (dict(S=-1), E_SHAPE), (dict(K=0), E_SHAPE), (dict(K=4097), E_SHAPE),
                 (dict(min_silence_frames=3), E_SHAPE), (dict(pad=-1), E_SHAPE), (dict(pad=65537), E_SHAPE), (dict(max_samples=0), E_SHAPE),
                 (dict(target_samples=-1), E_SHAPE), (dict(min_samples=-1), E_SHAPE), (dict(ld_audio=8191), E_SHAPE),
                 (dict(ref_mode=2), E_SHAPE), (dict(factor=-1.0), E_SHAPE), (dict(factor=float("nan")), E_SHAPE),
                 (dict(ref_mode=1, ref=-1.0), E_SHAPE),
                 (dict(workspace_bytes=runtime.segment_workspace_bytes(2, 8192) - 1), E_ALIGN), (dict(workspace=ctypes.c_void_p((1 << 20) + 4)), E_ALIGN)
                 ] + [({name: None}, E_NULL) for name in ("audio", "audio_len", "segments", "flags", "count", "wanted", "frames",
                                                          "speech_frames", "speech_power", "noise_power", "workspace")]
GATHER_REFUSALS = [(dict(B=65536), E_SHAPE), (dict(S=-1), E_SHAPE), (dict(S_out=-1), E_SHAPE), (dict(K=0), E_SHAPE), (dict(K=4097), E_SHAPE),
                   (dict(R=-1), E_SHAPE), (dict(R=65536), E_SHAPE), (dict(drop=4), E_SHAPE), (dict(drop=-1), E_SHAPE),
                   (dict(ld_audio=8191), E_SHAPE), (dict(ld_out=63), E_SHAPE),
                   (dict(out=ctypes.c_void_p((1 << 20) + 4 * 8191)), E_SHAPE),                       # the last sample of audio's first row
                   (dict(out=ctypes.c_void_p((1 << 20) - 4 * (3 * 64 + 63))), E_SHAPE),              # out's last sample is audio's first
                   ] + [({name: None}, E_NULL) for name in ("audio", "segments", "flags", "count", "out", "out_len", "item", "index",
                                                            "bounds", "row_flags", "rows", "rows_wanted")]


def test_argument_errors_without_gpu():
    lib = runtime.lib()
    I32, I64, F64, P = ctypes.c_int32, ctypes.c_int64, ctypes.c_double, ctypes.c_void_p
    assert runtime.SIGNATURES["ispk_segment_plan"] == [P, I64, P, F64, I32, F64, I32, I32, I64, I64, I64] + [P] * 9 + [I64, I32, I32, I32, P]
    assert runtime.SIGNATURES["ispk_segment_gather_f32"] == [P, I64, P, P, P, I32, P, I64] + [P] * 7 + [I32] * 5 + [P]
    assert runtime.SIGNATURES["ispk_segment_workspace_bytes"] == [I32, I32, P]
    for B, S in ((0, 0), (1, 0), (1, 1), (2, 8192), (3, 8193), (7, 2 ** 31 - 1), (65535, 441000)):
        n = ctypes.c_int64(-1)
        assert lib.ispk_segment_workspace_bytes(B, S, ctypes.byref(n)) == 0 and n.value == runtime.segment_workspace_bytes(B, S), (B, S)
    assert lib.ispk_segment_workspace_bytes(65536, 8, ctypes.byref(n)) == E_SHAPE and lib.ispk_segment_workspace_bytes(1, 8, None) == E_NULL
    assert lib.ispk_segment_plan(*_plan_args(B=0, audio=None, workspace=None)) == 0           # a no-op: no pointer is looked at
    assert lib.ispk_segment_plan(*_plan_args(B=0, K=0)) == E_SHAPE                            # the scalars are checked first
    for kw, code in PLAN_REFUSALS:
        assert lib.ispk_segment_plan(*_plan_args(**kw)) == code, kw
        assert b"ispk_segment_plan" in lib.ispk_last_error_string()
    for kw, code in GATHER_REFUSALS:
        assert lib.ispk_segment_gather_f32(*_gather_args(**kw)) == code, kw
        assert b"ispk_segment_gather_f32" in lib.ispk_last_error_string()


def test_python_face():
    from isp_tts_amd.bindings import audio
    names = {"segment_plan", "segment_gather", "segment_workspace_bytes", "SEGMENT_MAX_SEGMENTS", "SEGMENT_MAX_ROWS", "SEGMENT_MAX_PAD",
             "SEGMENT_FLAGS"}
    assert names <= set(audio.__all__) and names <= set(runtime.__dict__)
    assert runtime.SEGMENT_MAX_SEGMENTS == 4096 and runtime.SEGMENT_FLAGS == {"over": 1, "short": 2, "cut": 4}
    assert hasattr(data, "Segmenter")
    a = torch.zeros((2, 64))
    with pytest.raises(ValueError, match="max_segments"):
        runtime.segment_plan(a, torch.zeros(2, dtype=torch.int64), 1e-4, 0, 0.0, 1, 4, 100, 200, 10, 0)
    with pytest.raises(ValueError, match="rows"):
        runtime.segment_gather(a, torch.zeros((2, 4, 2), dtype=torch.int64), torch.zeros((2, 4), dtype=torch.int32),
                               torch.zeros(2, dtype=torch.int32), 0, -1, 16)
    with pytest.raises(ValueError, match="flags"):
        runtime.segment_gather(a, torch.zeros((2, 4, 2), dtype=torch.int64), torch.zeros((2, 5), dtype=torch.int32),
                               torch.zeros(2, dtype=torch.int32), 0, 4, 16)
    with pytest.raises(runtime.IspkError, match="GPU tensors"):
        runtime.segment_gather(a, torch.zeros((2, 4, 2), dtype=torch.int64), torch.zeros((2, 4), dtype=torch.int32),
                               torch.zeros(2, dtype=torch.int32), 0, 4, 16)
