"""CPU: the noise reducer's float64 restatement (tests/noise_reference.py) does what the definition promises, the constructor of
data.NoiseReducer validates, and the four entry points of csrc/noise.hip are exported, bound from the header and refuse bad
arguments before any launch.

What "changes the bursts by less than the noise it removed" is held to.  Without smoothing the gain of a bin depends on that bin
alone: inside a burst the partials keep a gain of almost 1 and every other bin loses its noise, so the RMS change inside the
bursts is below the RMS of what was removed from the pauses (measured 6.63e-4 against 6.93e-4).  With smoothing a cell shares the
gain of its neighbours, so the skirt of a partial is pulled towards the floor next to it: the RMS change inside the bursts then
exceeds the removed noise (5.0e-3) by construction of the definition, and the check is on the level - the bursts' power moves by
less than the 1 dB of slack that the pause check has (measured 0.094 dB), against 11.2 dB in the pauses."""
import ctypes

import numpy as np
import pytest

import noise_reference as R
from isp_tts_amd import runtime
from isp_tts_amd.data import NoiseReducer

N_SIG, FACTOR, GUARD, MIN_FRAMES = 24576, 1e-4, 2, 8
REDUCE_DB = 12.0
G_MIN = 10.0 ** (-REDUCE_DB / 20.0)
BURSTS = [(s, s + 1536) for s in range(1024, N_SIG, 6144)]
_CACHE = {}


def signal():
    if not _CACHE:
        x = R.make_signal(N_SIG, 1)
        _CACHE.update(x=x, item=R.profile_item(x, N_SIG, N_SIG, FACTOR, "max", GUARD, MIN_FRAMES))
    return _CACHE["x"], _CACHE["item"]


def db(a, b):
    return 10.0 * np.log10(a / b)


def test_signal_has_a_profile():
    x, it = signal()
    m, thr = R.margin(x, N_SIG, FACTOR, "max")
    assert m > 0.5 and thr > 0                              # pauses far below, bursts far above
    assert it["flags"] == 0 and it["frames"] == 1 + N_SIG // 256 and it["noise_frames"] >= 4 * MIN_FRAMES
    inside = R.burst_mask(N_SIG, BURSTS, 0)
    for f in np.flatnonzero(it["mask"]):                    # a noise frame touches no burst
        assert not inside[256 * (f - 2):256 * (f - 2) + 1024].any(), f
    # white noise of sigma 1e-3 under a Hann window: E |X|^2 = sigma^2 sum w^2 = 3.84e-4 in every bin but the two real ones
    assert 0.8 < it["noise"][1:-1].mean() / (1e-6 * 384.0) < 1.25


def test_over_zero_is_the_identity():
    x, it = signal()
    y = R.reduce_item(x, it["noise"], 0.0, G_MIN, 2, 2)
    assert np.abs(y - x).max() <= 1e-12 * np.abs(x).max()


def test_pauses_drop_and_bursts_stay():
    x, it = signal()
    pause, burst = ~R.burst_mask(N_SIG, BURSTS), R.burst_mask(N_SIG, BURSTS, -64)
    assert pause.sum() > 4000 and burst.sum() > 4000
    y = R.reduce_item(x, it["noise"], 2.0, G_MIN, 2, 2)     # the defaults
    drop = db((x[pause] ** 2).mean(), (y[pause] ** 2).mean())
    moved = abs(db((x[burst] ** 2).mean(), (y[burst] ** 2).mean()))
    print(f"defaults: pauses lowered by {drop:.2f} dB, bursts moved by {moved:.3f} dB")
    assert drop >= REDUCE_DB - 1.0
    assert moved < 1.0 and moved < drop
    y0 = R.reduce_item(x, it["noise"], 2.0, G_MIN, 0, 0)    # the raw gain alone
    removed = np.sqrt(((x - y0)[pause] ** 2).mean())
    changed = np.sqrt(((x - y0)[burst] ** 2).mean())
    print(f"unsmoothed: removed {removed:.3e} RMS from the pauses, changed the bursts by {changed:.3e} RMS")
    assert changed < removed


def test_separable_and_2d_smoothing_agree():
    g = np.random.default_rng(0).random((9, 513))
    for Tt, Fk in ((0, 0), (2, 2), (1, 8), (2, 8), (0, 3), (2, 0)):
        assert np.abs(R.smooth_2d(g, Tt, Fk) - R.smooth_separable(g, Tt, Fk)).max() <= 1e-13, (Tt, Fk)
    one = np.random.default_rng(1).random((1, 513))          # a single frame: the time weights renormalise to 1
    assert np.abs(R.smooth_2d(one, 2, 2) - R.smooth_separable(one, 0, 2)).max() <= 1e-13
    assert np.array_equal(R.smooth_2d(g, 0, 0), g)


def test_reference_flags_and_copies():
    x, it = signal()
    short = R.profile_item(x, 512, N_SIG, FACTOR, "max", GUARD, MIN_FRAMES)
    assert short["flags"] == R.SHORT | R.NO_PROFILE and short["frames"] == 0 and not short["noise"].any()
    busy = R.profile_item(x[1024:2560], 1536, 1536, FACTOR, "max", GUARD, MIN_FRAMES)   # a burst alone: no pause
    assert busy["flags"] == R.NO_PROFILE and busy["noise_frames"] == 0 and not busy["noise"].any()
    audio = np.stack([x[:4096], x[:4096], x[:4096], x[:4096]])
    out = R.reduce_batch(audio, [4096, 300, 4096, 4097], it["noise"][None], 2.0, G_MIN, 2, 2, index=[0, 0, 1, 0])
    assert np.array_equal(out[1, :300], x[:300]) and not out[1, 300:].any()
    assert np.array_equal(out[2], x[:4096]) and not out[3].any()
    assert np.abs(out[0] - x[:4096]).max() > 1e-3 * np.abs(x).max()


def test_constructor_validation():
    nr = NoiseReducer(22050)
    assert nr.factor == 1e-4 and nr.guard_frames == 5 and nr.min_noise_frames == 8
    assert nr.over == 2.0 and abs(nr.g_min - G_MIN) < 1e-15 and (nr.smooth_frames, nr.smooth_bins) == (2, 2)
    assert nr.tables.dtype.is_floating_point and nr.tables.numel() == 5120
    assert NoiseReducer(16000, ref=0.5, guard_ms=0.0, reduce_db=0.0).g_min == 1.0
    bad = [dict(sample_rate=0), dict(sample_rate=22050.5), dict(top_db=0.0), dict(top_db=float("inf")), dict(ref="min"), dict(ref=0.0),
           dict(guard_ms=-1.0), dict(guard_ms=float("nan")), dict(guard_ms=1e9), dict(min_noise_frames=0), dict(min_noise_frames=2.5),
           dict(over=-0.1), dict(over=float("inf")), dict(reduce_db=-1.0), dict(reduce_db=float("nan")), dict(smooth_frames=3),
           dict(smooth_frames=-1), dict(smooth_frames=1.5), dict(smooth_bins=9), dict(smooth_bins=-1)]
    for kw in bad:
        with pytest.raises(ValueError):
            NoiseReducer(**{"sample_rate": 22050, **kw})
    import torch
    with pytest.raises(runtime.IspkError, match="GPU tensors"):
        nr.profile(torch.zeros(1, 2048), torch.tensor([2048]))
    with pytest.raises(runtime.IspkError, match="GPU tensors"):
        nr.apply(torch.zeros(1, 2048), torch.tensor([2048]), torch.zeros(1, 513, dtype=torch.float64))
    with pytest.raises(ValueError, match="fp32"):
        nr.profile(torch.zeros(1, 2048, dtype=torch.float64), torch.tensor([2048]))
    out = nr.empty_outputs(3, samples=5000)
    assert set(out) == {"noise", "noise_frames", "frames", "flags", "work", "audio"} and out["noise"].shape == (3, 513)
    assert out["work"].numel() == runtime.noise_workspace_bytes(3, 5000) and out["audio"].shape == (3, 5000)


SYMBOLS = ("ispk_noise_tile_samples", "ispk_noise_workspace_bytes", "ispk_noise_profile_f64", "ispk_noise_reduce_f32")


def test_symbols_are_exported_and_bound_from_the_header():
    P, I32, I64, F64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    known = {
        "ispk_noise_tile_samples": [],
        "ispk_noise_workspace_bytes": [I32, I32, P],
        "ispk_noise_profile_f64": [P, I64, P, P, F64, I32, F64, I32, I32, P, P, P, P, P, I64, I32, I32, P],
        "ispk_noise_reduce_f32": [P, I64, P, P, P, I32, P, P, F64, F64, I32, I32, P, I64, I32, I32, P],
    }
    handle = ctypes.CDLL(runtime.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(handle, name), f"{name} is missing from libispk.so"
        assert runtime.SIGNATURES[name] == known[name], name
        assert runtime.RESTYPES[name] is I32
    lib = runtime.lib()
    assert lib.ispk_noise_tile_samples() == runtime.NOISE_TILE_SAMPLES == 4096
    for B, S in ((1, 1), (3, 5000), (2, 4096), (64, 131072), (1, 1 << 24)):
        got = ctypes.c_int64(-1)
        assert lib.ispk_noise_workspace_bytes(B, S, ctypes.byref(got)) == 0
        assert got.value == runtime.noise_workspace_bytes(B, S), (B, S)


def test_argument_errors_without_gpu():
    lib = runtime.lib()
    E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(20)     # never dereferenced: the checks fail first
    B, S = 2, 8192
    need = runtime.noise_workspace_bytes(B, S)
    assert lib.ispk_noise_workspace_bytes(1, 1, None) == E_NULL
    assert lib.ispk_noise_workspace_bytes(65536, 1, one) == E_SHAPE and lib.ispk_noise_workspace_bytes(1, (1 << 24) + 1, one) == E_SHAPE
    prof = dict(audio=one, ld_audio=S, audio_len=one, tables=one, factor=1e-4, ref_mode=0, ref=0.0, guard=5, min_noise_frames=8,
                noise=one, noise_frames=one, frames=one, flags=one, workspace=one, workspace_bytes=need, B=B, S=S, stream=None)
    refused = [(dict(B=65536), E_SHAPE), (dict(S=-1), E_SHAPE), (dict(S=(1 << 24) + 1), E_SHAPE), (dict(ref_mode=2), E_SHAPE),
               (dict(factor=-1.0), E_SHAPE), (dict(factor=float("nan")), E_SHAPE), (dict(ref_mode=1, ref=-1.0), E_SHAPE),
               (dict(guard=-1), E_SHAPE), (dict(guard=65537), E_SHAPE), (dict(min_noise_frames=0), E_SHAPE), (dict(ld_audio=S - 1), E_SHAPE),
               (dict(workspace_bytes=need - 1), E_ALIGN), (dict(workspace=odd), E_ALIGN)]
    refused += [({k: None}, E_NULL) for k in ("audio", "audio_len", "tables", "noise", "noise_frames", "frames", "flags", "workspace")]
    for kw, code in refused:
        assert lib.ispk_noise_profile_f64(*{**prof, **kw}.values()) == code, kw
    assert b"ispk_noise_profile_f64" in lib.ispk_last_error_string()
    red = dict(audio=one, ld_audio=S, audio_len=one, tables=one, noise=one, P=1, index=None, flags=None, over=2.0, g_min=0.25,
               smooth_frames=2, smooth_bins=2, out=ctypes.c_void_p(32), ld_out=S, B=B, S=S, stream=None)
    refused = [(dict(B=65536), E_SHAPE), (dict(B=-1), E_SHAPE), (dict(S=(1 << 31) - 8192), E_SHAPE), (dict(P=0), E_SHAPE),
               (dict(ld_audio=S - 1), E_SHAPE), (dict(ld_out=S - 1), E_SHAPE), (dict(out=one), E_SHAPE), (dict(over=-1.0), E_SHAPE),
               (dict(over=float("inf")), E_SHAPE), (dict(over=float("nan")), E_SHAPE), (dict(g_min=0.0), E_SHAPE), (dict(g_min=1.5), E_SHAPE),
               (dict(g_min=float("nan")), E_SHAPE), (dict(smooth_frames=3), E_SHAPE), (dict(smooth_frames=-1), E_SHAPE),
               (dict(smooth_bins=9), E_SHAPE), (dict(smooth_bins=-1), E_SHAPE)]
    refused += [({k: None}, E_NULL) for k in ("audio", "tables", "noise", "out")]
    for kw, code in refused:
        assert lib.ispk_noise_reduce_f32(*{**red, **kw}.values()) == code, kw
    assert b"ispk_noise_reduce_f32" in lib.ispk_last_error_string()


def test_zero_sized_batches_are_noops():
    lib = runtime.lib()
    one = ctypes.c_void_p(16)
    for B, S in ((0, 8192), (2, 0)):
        assert lib.ispk_noise_profile_f64(one, S, one, one, 1e-4, 0, 0.0, 5, 8, one, one, one, one, one, 0, B, S, None) == 0
        assert lib.ispk_noise_reduce_f32(one, S, one, one, one, 1, None, None, 2.0, 0.25, 2, 2, one, S, B, S, None) == 0
    got = ctypes.c_int64(-1)
    assert lib.ispk_noise_workspace_bytes(0, 0, ctypes.byref(got)) == 0 and got.value == 0
