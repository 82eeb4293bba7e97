"""The segmenter on the GPU (ispk_segment_plan, ispk_segment_gather_f32, data.Segmenter) against its numpy restatement
(tests/segmenter_reference.py) on the recordings of tests/segmenter_cases.py: integers with ==, audio by its bytes.

tests/test_segmenter_host.py asserts that every recording keeps its frame powers at least 2^-30 (relative) away from the
threshold, a million times what any order of summation can move them, so the integers are comparable at all.

Levels.  speech_power / noise_power against the float64 reference, relative bound (n + 300) 2^-53 with n = the segment's frames:
n - 1 additions of non-negative terms in any order account for (n - 1) 2^-53, each p_t carries at most (256 + 3 + 1) 2^-53 from
its hop sums (the reference's are exactly rounded), the rest covers the divisions.  test_plan_against_reference and
test_long_recording print the worst ratio to the bound; DESIGN.md 4.30 records it."""
import ctypes

import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

import segmenter_cases as C
import segmenter_reference as R
from isp_tts_amd import graph, runtime
from isp_tts_amd.data import AcousticFeatures, AudioConditioner, Segmenter

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PLAN_INT = ("segments", "flags", "count", "wanted", "frames", "speech_frames")
PLAN_ALL = PLAN_INT + ("speech_power", "noise_power")
ROW_ALL = ("audio", "audio_len", "item", "index", "bounds", "row_flags", "rows", "rows_wanted")
DROPS = {(): 0, ("over",): 1, ("over", "short"): 3}


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


def segmenter(config="max", K=C.K_SMALL, drop=("over", "short")):
    cfg = C.CONFIGS[config]
    seg = Segmenter(C.RATE, top_db=C.TOP_DB, ref=cfg["ref"], max_segments=K, drop=drop)
    assert seg.factor == C.FACTOR
    seg.pad_frames = cfg["pad_frames"]
    for k, v in C.BUDGET.items():
        setattr(seg, k, v)
    return seg


_DEVICE = {}


def on_device(batch):
    """The batch on the GPU, made once: rows at a stride above S (a multiple of four floats, the base 16-byte aligned), NaN
    behind every item and between the rows."""
    if batch not in _DEVICE:
        c = C.small() if batch == "small" else C.long()
        B, S = c["audio"].shape
        LD = (S + 3) // 4 * 4 + 4
        full = torch.full((B, LD), float("nan"), device=DEV)
        full[:, :S] = torch.from_numpy(c["audio"]).to(DEV)
        lens = torch.from_numpy(c["lens"]).to(DEV)
        torch.cuda.synchronize()
        assert full.data_ptr() % 16 == 0 and full[:, :S].stride(0) == LD > S
        _DEVICE[batch] = dict(full=full, audio=full[:, :S], lens=lens, B=B, S=S, LD=LD)
    return _DEVICE[batch]


def check_plan(got, ref, what):
    """Integers exactly; the levels within (n + 300) 2^-53.  Returns the worst ratio to that bound."""
    for k in PLAN_INT:
        assert np.array_equal(host(got[k]), ref[k]), (what, k)
    worst = 0.0
    frames = ref["frames"]
    for k in ("speech_power", "noise_power"):
        g, r = host(got[k]), ref[k]
        assert np.array_equal(g == 0.0, r == 0.0), (what, k)                   # an empty set gives exactly 0, nothing else does
        nz = r != 0.0
        ratio = np.abs(g[nz] - r[nz]) / r[nz] / ((frames[nz] + 300) * 2.0 ** -53)
        if ratio.size:
            worst = max(worst, float(ratio.max()))
    assert worst <= 1.0, (what, worst)
    return worst


def check_rows(got, ref, what):
    for k in ROW_ALL:
        assert bits(got[k]) == ref[k].tobytes(), (what, k)


# ------------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("config", list(C.CONFIGS))
def test_plan_against_reference(config):
    d = on_device("small")
    _, ref = C.reference("small", config)
    got = segmenter(config).plan(d["audio"], d["lens"])
    torch.cuda.synchronize()
    assert set(got) == set(PLAN_ALL)
    worst = check_plan(got, ref, config)
    print(f"{config}: {int(ref['count'].sum())} segments stored of {int(ref['wanted'].sum())}; levels at worst {worst:.3f} of the bound")


@pytest.mark.parametrize("drop", list(DROPS))
def test_gather_against_reference(drop):
    d, c = on_device("small"), C.small()
    _, ref = C.reference("small", "max")
    seg = segmenter("max", drop=drop)
    assert seg.drop_mask == DROPS[drop]
    S_out = 40 * C.H
    for rows in (16, 96):                                                       # fewer rows than segments, and rows to spare
        want = R.gather(c["clean"], ref, DROPS[drop], rows, S_out)
        r = seg(d["audio"], d["lens"], rows=rows, samples=S_out)
        torch.cuda.synchronize()
        assert set(r) == set(PLAN_ALL) | set(ROW_ALL)
        check_plan(r, ref, drop)
        check_rows(r, want, (drop, rows))
        assert (want["rows_wanted"][0] > rows) == (rows == 16)
        if rows == 96:
            assert (want["item"][want["rows"][0]:] == -1).all() and (want["row_flags"] & R.CUT).any()
    flags = want["row_flags"][:want["rows"][0]]
    assert not (flags & DROPS[drop]).any() and (drop != () or ((flags & R.OVER).any() and (flags & R.SHORT).any()))
    # samples defaults to max_samples
    r = seg(d["audio"], d["lens"], rows=4)
    assert r["audio"].shape == (4, C.BUDGET["max_samples"])
    check_rows(r, R.gather(c["clean"], ref, DROPS[drop], 4, C.BUDGET["max_samples"]), (drop, "default"))


def test_long_recording():
    """8,600 frames and some 260 pauses: every per-item pass strides more than once (the frame passes, the candidate pass with
    its chunks of 8,192 frames, the choice with its tiles of 128 candidates - a pause is passed over at a tile's last slot), and
    the level pass has some 170 segments for its waves."""
    d, c = on_device("long"), C.long()
    for config in ("max", "const"):
        _, ref = C.reference("long", config)
        seg = segmenter(config, K=C.K_LONG, drop=())
        r = seg(d["audio"], d["lens"], rows=200, samples=80 * C.H)
        torch.cuda.synchronize()
        worst = check_plan(r, ref, config)
        check_rows(r, R.gather(c["clean"], ref, 0, 200, 80 * C.H), config)
        print(f"long, {config}: {int(ref['wanted'][0])} segments; levels at worst {worst:.3f} of the bound")


# ------------------------------------------------------------------------------------------------ bit for bit
def test_alone_in_a_batch_permuted_repeated():
    d = on_device("small")
    seg = segmenter("max", drop=())
    plan = {k: v.clone() for k, v in seg.plan(d["audio"], d["lens"]).items()}
    again = seg.plan(d["audio"], d["lens"])
    for k in PLAN_ALL:
        assert bits(again[k]) == bits(plan[k]), k
    perm = torch.from_numpy(np.random.default_rng(3).permutation(d["B"])).to(DEV)
    moved = seg.plan(d["audio"][perm].contiguous(), d["lens"][perm].contiguous())
    for k in PLAN_ALL:
        assert bits(moved[k]) == bits(plan[k][perm]), k
    for name in ("len257", "gap_exact", "look_again", "at_max", "many", "ragged", "silent"):
        b = C.NAMES.index(name)
        one = seg.plan(d["audio"][b:b + 1], d["lens"][b:b + 1])
        for k in PLAN_ALL:
            assert bits(one[k][0]) == bits(plan[k][b]), (name, k)
    # the rows of an item alone are its rows in the batch
    b = C.NAMES.index("many")
    whole = seg(d["audio"], d["lens"], rows=96, samples=48 * C.H)
    sel = host(whole["item"]) == b
    one = seg(d["audio"][b:b + 1], d["lens"][b:b + 1], rows=int(sel.sum()), samples=48 * C.H)
    torch.cuda.synchronize()
    assert sel.sum() == C.K_SMALL and int(one["rows"][0]) == C.K_SMALL
    for k in ("audio", "audio_len", "index", "bounds", "row_flags"):
        assert bits(one[k]) == host(whole[k])[sel].tobytes(), k


def test_row_stride_and_misaligned_base():
    """The batch at a stride that is no multiple of four floats from a base 4 bytes off a 16-byte boundary takes the scalar loads;
    `out` likewise.  The same values either way, and nothing outside `out` is written."""
    d = on_device("small")
    B, S, LD = d["B"], d["S"], d["LD"]
    seg = segmenter("max", drop=())
    rows, S_out = 24, 40 * C.H
    base = seg(d["audio"], d["lens"], rows=rows, samples=S_out)
    shifted = torch.full((B * (LD + 1) + 1,), float("nan"), device=DEV)
    view = shifted[1:].view(B, LD + 1)[:, :S]
    view.copy_(d["audio"])
    assert view.data_ptr() % 16 == 4 and view.stride(0) % 4 == 1
    wide = torch.full((rows * (S_out + 5) + 1,), 7.0, device=DEV)
    out = seg.empty_outputs(B, rows, S_out, DEV)
    out["audio"] = wide[1:].view(rows, S_out + 5)[:, :S_out]
    r = seg(view, d["lens"], out=out)
    torch.cuda.synchronize()
    assert r["audio"].data_ptr() == out["audio"].data_ptr() and r["audio"].data_ptr() % 16 == 4
    for k in PLAN_ALL + ROW_ALL:
        assert bits(r[k].contiguous()) == bits(base[k]), k
    pad = wide[1:].view(rows, S_out + 5)[:, S_out:]
    assert bits(wide[:1]) == bits(torch.full((1,), 7.0)) and bits(pad.contiguous()) == bits(torch.full((rows, 5), 7.0))


# ------------------------------------------------------------------------------------------------ no ATen op, graph capture
def test_no_aten_op_and_graph_replay():
    d = on_device("small")
    seg = segmenter("max")
    rows, S_out = 32, 48 * C.H
    eager = {k: v.clone() for k, v in seg(d["audio"], d["lens"], rows=rows, samples=S_out).items()}
    out = seg.empty_outputs(d["B"], rows, S_out, DEV, recording_samples=d["S"])
    spy = Spy()
    with spy:
        r = seg(d["audio"], d["lens"], out=out)
    torch.cuda.synchronize()
    assert spy.seen == [], spy.seen
    assert set(r) == set(PLAN_ALL) | set(ROW_ALL) and all(r[k] is out[k] for k in r)
    for k in r:
        assert bits(r[k]) == bits(eager[k]), k
    static = seg.empty_outputs(d["B"], rows, S_out, DEV)                        # (the warm-up calls add "work")
    g = graph.GraphedCall(lambda: seg(d["audio"], d["lens"], out=static))
    for _ in range(2):
        for k in PLAN_ALL + ROW_ALL:
            static[k].fill_(3)
        torch.cuda.synchronize()
        spy = Spy()
        with spy:
            r = g.replay()
        torch.cuda.synchronize()
        assert spy.seen == [], spy.seen
        for k in r:
            assert bits(r[k]) == bits(eager[k]), k


# ------------------------------------------------------------------------------------------------ beside the conditioner
@pytest.mark.parametrize("config", ["max", "const"])
def test_ends_are_the_conditioners_bounds(config):
    d = on_device("small")
    cfg = C.CONFIGS[config]
    plan = segmenter(config).plan(d["audio"], d["lens"])
    cond = AudioConditioner(C.RATE, target_lufs=None, top_db=C.TOP_DB, pad_frames=cfg["pad_frames"], ref=cfg["ref"])
    bounds = host(cond(d["audio"], d["lens"])["bounds"])
    items, _ = C.reference("small", config)
    seen = 0
    for b, it in enumerate(items):
        if len(it["candidates"]) == 0:                                          # no qualifying pause: at most one segment
            seen += 1
            count = int(plan["count"][b])
            want = tuple(host(plan["segments"])[b, 0]) if count else (0, 0)
            assert count <= 1 and tuple(bounds[b]) == want == (it["first"], it["last"]), C.NAMES[b]
    assert seen >= 12


def test_chain_in_one_graph():
    """seg -> AudioConditioner -> AcousticFeatures as one captured graph; every used row is conditioned as that piece alone is."""
    d = on_device("small")
    seg = segmenter("max", drop=("over",))
    cond = AudioConditioner(C.RATE, top_db=60.0)
    feats = AcousticFeatures(sample_rate=C.RATE, f_max=4000.0, pitch=False)
    rows, S_out = 64, C.BUDGET["max_samples"]
    o_seg = seg.empty_outputs(d["B"], rows, S_out, DEV, recording_samples=d["S"])
    o_cond, o_feat = cond.empty_outputs(rows, S_out, DEV), feats.empty_outputs(rows, S_out, DEV)
    cond.device_tables(DEV), feats.device_tables(DEV)

    def chain():
        r = seg(d["audio"], d["lens"], out=o_seg)
        c = cond(r["audio"], r["audio_len"], out=o_cond)
        return r, c, feats(c["audio"], c["audio_len"], out=o_feat)

    g = graph.GraphedCall(chain)
    for t in (o_cond["bounds"], o_cond["loudness"], o_feat["mel_len"]):
        t.fill_(-1)
    r, c, f = g.replay()
    torch.cuda.synchronize()
    used = int(r["rows"][0])
    item, bnd, n = host(r["item"]), host(r["bounds"]), host(r["audio_len"])
    want = R.gather(C.small()["clean"], C.reference("small", "max")[1], 1, rows, S_out)
    check_rows(r, want, "chain")
    assert used == want["rows"][0] == want["rows_wanted"][0] < rows and not (host(r["row_flags"]) & R.CUT).any()
    finite = 0
    for row in range(used):
        b, s = int(item[row]), int(bnd[row, 0])
        piece = d["audio"][b:b + 1, s:s + int(n[row])]
        alone = cond(piece, torch.tensor([int(n[row])], dtype=torch.int64, device=DEV))
        assert bits(alone["bounds"][0]) == bits(c["bounds"][row]) and bits(alone["loudness"][0]) == bits(c["loudness"][row]), row
        finite += bool(torch.isfinite(c["loudness"][row]))
    assert finite >= 8
    assert bits(c["audio_len"][used:]) == bits(torch.zeros(rows - used, dtype=torch.int64))
    assert (host(f["mel_len"])[:used] == [runtime.feature_frames(int(v)) for v in host(c["audio_len"])[:used]]).all()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_launch_nothing():
    lib = runtime.lib()
    B, S, K, R_, S_out = 2, 8192, 8, 4, 64
    audio = torch.zeros((B, S), device=DEV)
    lens = torch.full((B,), S, dtype=torch.int64, device=DEV)
    seg = Segmenter(C.RATE, max_segments=K)
    out = seg.empty_outputs(B, R_, S_out, DEV, recording_samples=S)
    for t in out.values():
        t.fill_(5)
    torch.cuda.synchronize()
    before = {k: bits(v) for k, v in out.items()}
    p = lambda k: ctypes.c_void_p(out[k].data_ptr())                            # noqa: E731
    plan = dict(audio=ctypes.c_void_p(audio.data_ptr()), ld_audio=S, audio_len=ctypes.c_void_p(lens.data_ptr()), factor=1e-4, ref_mode=0,
                ref=0.0, pad=1, min_silence_frames=4, target_samples=100, max_samples=200, min_samples=10, segments=p("segments"),
                flags=p("flags"), count=p("count"), wanted=p("wanted"), frames=p("frames"), speech_frames=p("speech_frames"),
                speech_power=p("speech_power"), noise_power=p("noise_power"), workspace=p("work"), workspace_bytes=out["work"].numel(),
                B=B, S=S, K=K, stream=None)
    gather = dict(audio=plan["audio"], ld_audio=S, segments=p("segments"), flags=p("flags"), count=p("count"), drop=3, out=p("audio"),
                  ld_out=S_out, out_len=p("audio_len"), item=p("item"), index=p("index"), bounds=p("bounds"), row_flags=p("row_flags"),
                  rows=p("rows"), rows_wanted=p("rows_wanted"), B=B, S=S, K=K, R=R_, S_out=S_out, stream=None)
    E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3
    refused = [(dict(B=65536), E_SHAPE), (dict(S=-1), E_SHAPE), (dict(K=0), E_SHAPE), (dict(K=4097), E_SHAPE),
               (dict(min_silence_frames=3), E_SHAPE), (dict(pad=-1), E_SHAPE), (dict(pad=65537), E_SHAPE), (dict(max_samples=0), E_SHAPE),
               (dict(target_samples=-1), E_SHAPE), (dict(min_samples=-1), E_SHAPE), (dict(ld_audio=S - 1), E_SHAPE),
               (dict(workspace_bytes=runtime.segment_workspace_bytes(B, S) - 1), E_ALIGN),
               (dict(workspace=ctypes.c_void_p(out["work"].data_ptr() + 4)), E_ALIGN)]
    refused += [({k: None}, E_NULL) for k in ("audio", "audio_len", "segments", "flags", "count", "wanted", "frames", "speech_frames",
                                              "speech_power", "noise_power", "workspace")]
    for kw, code in refused:
        assert lib.ispk_segment_plan(*{**plan, **kw}.values()) == code, kw
    refused = [(dict(B=65536), E_SHAPE), (dict(S=-1), E_SHAPE), (dict(S_out=-1), E_SHAPE), (dict(K=0), E_SHAPE), (dict(R=65536), E_SHAPE),
               (dict(drop=4), E_SHAPE), (dict(ld_audio=S - 1), E_SHAPE), (dict(ld_out=S_out - 1), E_SHAPE),
               (dict(out=ctypes.c_void_p(audio.data_ptr() + 4 * (S - 1))), E_SHAPE)]
    refused += [({k: None}, E_NULL) for k in ("audio", "segments", "flags", "count", "out", "out_len", "item", "index", "bounds",
                                              "row_flags", "rows", "rows_wanted")]
    for kw, code in refused:
        assert lib.ispk_segment_gather_f32(*{**gather, **kw}.values()) == code, kw
    assert lib.ispk_segment_plan(*{**plan, "B": 0}.values()) == 0               # a no-op
    torch.cuda.synchronize()
    for k, v in out.items():
        assert bits(v) == before[k], k
    with pytest.raises(runtime.IspkError, match="overlaps"):
        runtime.segment_gather(audio, out["segments"], out["flags"], out["count"], 0, 1, S, out=dict(audio=audio[:1]))
    # and the same arguments, accepted: silence gives no segment and unused rows
    assert lib.ispk_segment_plan(*plan.values()) == 0 and lib.ispk_segment_gather_f32(*gather.values()) == 0
    torch.cuda.synchronize()
    assert not host(out["count"]).any() and (host(out["item"]) == -1).all() and not host(out["audio"]).any()
    assert int(out["rows"][0]) == 0 and int(out["rows_wanted"][0]) == 0
