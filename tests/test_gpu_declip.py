"""The declipper on the GPU (ispk_declip_f64, data.Declipper) against its numpy restatement (tests/declip_reference.py) on the
batches of tests/declip_cases.py.

Integers, thr and flags with ==; clip_samples also against data.Screen on the same batch.  The restored samples: within one fp32
ulp of the reference's fp32 value, and at most 1 % of them not bit-equal - the bounds that the float64 reference itself keeps
against its longdouble run on these very batches (tests/test_declip_host.py asserts that on the CPU; it measured 0 % there).  The
kernel sums in another order than numpy, so it is held to the same bounds and not to equality.  The SDR over the unknown samples is
within 0.01 dB of the reference's own.  peak is exact for the device's own output.  Every sample that is not unknown keeps its
bits; everything from the length on is zero.  test_against_reference prints the measured share; DESIGN.md 4.35 records it."""
import numpy as np
import pytest
import torch

import declip_cases as C
import declip_reference as D
from isp_tts_amd import graph
from isp_tts_amd.data import AudioConditioner, Declipper, Screen
from torch.utils._python_dispatch import TorchDispatchMode

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("audio",) + tuple(D.DTYPES)


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


def declipper(config="default"):
    return Declipper(**{"rail": "max", **C.CONFIGS[config]})


_DEVICE = {}


def on_device():
    """The batch on the GPU, made once: rows at a stride above S (a multiple of four floats), garbage behind every item and
    between the rows."""
    if not _DEVICE:
        c = C.batch()
        B, S = c["audio"].shape
        LD = S + 8
        full = torch.full((B, LD), C.GARBAGE, device=DEV)
        full[:, :S] = torch.from_numpy(c["audio"]).to(DEV)
        lens = torch.from_numpy(c["lens"]).to(DEV)
        torch.cuda.synchronize()
        assert full[:, :S].stride(0) == LD > S
        _DEVICE.update(full=full, audio=full[:, :S], lens=lens, B=B, S=S, LD=LD)
    return _DEVICE


def prefilled(dc, B, S):
    out = dc.empty_outputs(B, DEV, samples=S)
    for v in out.values():
        v.view(torch.uint8).fill_(0x5b)                     # (every element is written)
    return out


def check(got, items, ref, audio_in, clean=None, what=""):
    """Everything against the reference; returns (restored samples, those not bit-equal)."""
    for k in D.DTYPES:
        assert host(got[k]).dtype == D.DTYPES[k] and got[k].shape == (len(items),), (what, k)
        if k != "peak":                                                         # (the device's own output's, below)
            assert np.array_equal(host(got[k]), ref[k]), (what, k, host(got[k]), ref[k])
    y = host(got["audio"])
    total = differ = 0
    for b, it in enumerate(items):
        n, kept = it["n"], it["kept"]
        assert not y[b, n:].any(), (what, b)
        same = y[b, :n].view(np.int32) == audio_in[b, :n].view(np.int32)
        assert same[~it["mask"]].all(), (what, b, "a sample outside the unknown runs moved")
        assert same[it["mask"] & ~kept].all(), (what, b, "a dense segment moved")
        fin = np.where(np.isfinite(y[b, :n]), y[b, :n], np.float32(0.0))
        assert host(got["peak"])[b] == (np.abs(fin).max() if n else np.float32(0.0)), (what, b)
        if not kept.any():
            continue
        u = D.ulps(y[b, :n][kept], it["audio"][:n][kept])
        assert u.max() <= 1, (what, b, int(u.max()))
        total, differ = total + int(kept.sum()), differ + int((u > 0).sum())
        if clean is not None:
            mine, theirs = D.sdr_db(clean[b, :n], y[b, :n], kept), D.sdr_db(clean[b, :n], it["audio"][:n], kept)
            assert abs(mine - theirs) <= 0.01, (what, b, mine, theirs)
    assert differ <= 0.01 * total, (what, differ, total)
    return total, differ


# ------------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("config", list(C.CONFIGS))
def test_against_reference(config):
    d, c = on_device(), C.batch()
    dc = declipper(config)
    out = prefilled(dc, d["B"], d["S"])
    got = dc(d["audio"], d["lens"], out=out)
    torch.cuda.synchronize()
    assert set(got) == set(KEYS) and all(got[k] is out[k] for k in got)
    items, ref = C.reference(config)
    total, differ = check(got, items, ref, c["audio"], c["clean"], config)
    print(f"{config}: {total} restored samples, {differ} ({100.0 * differ / max(total, 1):.3f} %) not bit-equal to the float64 reference")
    kw = C.CONFIGS[config]
    s = Screen(C.RATE, rail=kw.get("rail", "max"), min_run=kw.get("min_run", 3))(d["audio"], d["lens"], parts=1)
    torch.cuda.synchronize()
    assert np.array_equal(host(s["clip_samples"]), host(got["clip_samples"])), config
    assert bits(d["full"][:, d["S"]:]) == bits(torch.full((d["B"], d["LD"] - d["S"]), C.GARBAGE))      # the input is not written


def test_the_dense_limit():
    """256 unknown samples in a window are solved, 257 are left."""
    c = C.dense_limit()
    audio, lens = torch.from_numpy(c["audio"]).to(DEV), torch.from_numpy(c["lens"]).to(DEV)
    dc = declipper()
    got = dc(audio, lens, out=prefilled(dc, 3, 1024))
    torch.cuda.synchronize()
    assert host(got["windows"]).tolist() == [2, 0, 1] and host(got["dense"]).tolist() == [0, 2, 1]
    check(got, c["items"], c["ref"], c["audio"], what="dense limit")
    assert bits(got["audio"][1]) == bits(audio[1])


def test_a_clipped_sinusoid_is_left_as_it_is():
    y = C.sinusoid()
    audio, lens = torch.from_numpy(y[None]).to(DEV), torch.tensor([C.S], dtype=torch.int64, device=DEV)
    got = declipper()(audio, lens)
    torch.cuda.synchronize()
    assert bits(got["audio"]) == bits(audio)
    assert (int(got["dense"][0]), int(got["windows"][0]), int(got["restored"][0]), int(got["flags"][0])) == (8, 0, 0, 2)


def test_screen_flags_skip_clean_items():
    """flags= with one item's bit cleared: that item is a copy bit for bit, with flag 4; the others as without flags."""
    d, c = on_device(), C.batch()
    s = Screen(C.RATE)(d["audio"], d["lens"], parts=1)
    torch.cuda.synchronize()
    assert (host(s["flags"]) & 1).tolist() == [1, 1, 1]
    flags = s["flags"].clone()
    flags[1] &= ~1
    dc = declipper()
    got = dc(d["audio"], d["lens"], flags=flags, out=prefilled(dc, d["B"], d["S"]))
    torch.cuda.synchronize()
    items, ref = C.reference("default", skip=(1,))
    assert ref["flags"].tolist() == [1, 4, 1] and ref["clip_samples"][1] == 0
    check(got, items, ref, c["audio"], c["clean"], "skip")
    n = C.LENS[1]
    assert bits(got["audio"][1, :n]) == bits(d["audio"][1, :n])                 # (the NaN and the Inf among them)
    assert np.isnan(host(got["audio"])[1, 100]) and np.isinf(host(got["audio"])[1, 101])


def test_zero_and_empty_items():
    S = 1500
    audio = torch.zeros((4, S), device=DEV)
    audio[2:] = 0.25
    lens = torch.tensor([1000, 0, -5, S + 1], dtype=torch.int64, device=DEV)
    dc = declipper()
    got = dc(audio, lens, out=prefilled(dc, 4, S))
    torch.cuda.synchronize()
    assert host(got["audio_len"]).tolist() == [1000, 0, 0, 0]
    for k in KEYS:
        assert k == "audio_len" or not host(got[k]).any(), k


# ------------------------------------------------------------------------------------------------ bit for bit
def test_alone_strided_repeated():
    d = on_device()
    B, S, LD = d["B"], d["S"], d["LD"]
    dc = declipper()
    base = {k: v.clone() for k, v in dc(d["audio"], d["lens"]).items()}
    again = dc(d["audio"], d["lens"])
    for k in KEYS:
        assert bits(again[k]) == bits(base[k]), k
    for b in range(B):                                                          # every item alone, cut to its own length
        n = C.LENS[b]
        one = dc(d["audio"][b:b + 1, :n], d["lens"][b:b + 1])
        for k in KEYS:
            assert bits(one[k][0]) == bits(base[k][b, :n] if k == "audio" else base[k][b]), (b, k)
    # odd strides from bases 4 bytes off an 8-byte boundary, in and out: the scalar loads and stores
    shifted = torch.full((B * (LD + 1) + 1,), C.GARBAGE, device=DEV)
    view = shifted[1:].view(B, LD + 1)[:, :S]
    view.copy_(d["audio"])
    target = torch.zeros((B * (S + 3) + 1,), device=DEV)[1:].view(B, S + 3)[:, :S]
    assert view.data_ptr() % 8 == 4 and view.stride(0) % 2 == 1 and target.data_ptr() % 8 == 4
    other = dc(view, d["lens"], out=dict(audio=target))
    torch.cuda.synchronize()
    assert other["audio"] is target
    for k in KEYS:
        assert bits(other[k]) == bits(base[k]), k


def test_no_aten_op_graph_replay_and_aliasing():
    d = on_device()
    dc = declipper()
    eager = {k: v.clone() for k, v in dc(d["audio"], d["lens"]).items()}
    out = dc.empty_outputs(d["B"], DEV, samples=d["S"])
    spy = Spy()
    with spy:
        r = dc(d["audio"], d["lens"], out=out)
    torch.cuda.synchronize()
    assert spy.seen == [], spy.seen
    for k in r:
        assert bits(r[k]) == bits(eager[k]), k
    static = dc.empty_outputs(d["B"], DEV, samples=d["S"])
    g = graph.GraphedCall(lambda: dc(d["audio"], d["lens"], out=static))
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
    contiguous = d["audio"].contiguous()
    for alias in (contiguous, contiguous.view(-1)[1:-1][:(d["B"] - 1) * d["S"]].view(d["B"] - 1, d["S"])):
        with pytest.raises(ValueError, match="out of place"):
            dc(contiguous[:alias.shape[0]], d["lens"][:alias.shape[0]], out=dict(audio=alias))


def test_screen_declipper_conditioner_as_one_graph():
    d = on_device()
    B, S = d["B"], d["S"]
    screen, dc, cond = Screen(C.RATE), declipper(), AudioConditioner(C.RATE, target_lufs=None, top_db=None)
    s_out, d_out, c_out = screen.empty_outputs(B, DEV, samples=S), dc.empty_outputs(B, DEV, samples=S), cond.empty_outputs(B, S, DEV)

    def chain():
        s = screen(d["audio"], d["lens"], out=s_out, parts=1)
        r = dc(d["audio"], d["lens"], flags=s["flags"], out=d_out)
        return r, cond(r["audio"], r["audio_len"], out=c_out)
    r, c = chain()
    torch.cuda.synchronize()
    eager = {k: v.clone() for k, v in r.items()}, {k: v.clone() for k, v in c.items()}
    g = graph.GraphedCall(chain)
    for t in list(d_out.values()) + list(c_out.values()):
        t.view(torch.uint8).fill_(0x5b)
    torch.cuda.synchronize()
    r, c = g.replay()
    torch.cuda.synchronize()
    for got, want in zip((r, c), eager):
        for k in want:
            assert bits(got[k]) == bits(want[k]), k
    items, ref = C.reference()
    check(r, items, ref, C.batch()["audio"], C.batch()["clean"], "chain")
    assert np.array_equal(host(c["audio_len"]), host(r["audio_len"])) and (host(c["gain"]) == 1.0).all()
    for b in (0, 2):                                                            # (item 1 holds a NaN; the shift alone: a copy)
        assert bits(c["audio"][b]) == bits(r["audio"][b]) and bits(c["peak"][b]) == bits(r["peak"][b]), b
    rows = dc.manifest(r, ["a", "b", "c"])
    assert [row["flags"] for row in rows] == [("restored",)] * 3 and rows[0]["restored"] == int(ref["restored"][0])
