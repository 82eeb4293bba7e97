"""The equalizer on the GPU (ispk_equalize_f32, data.Equalizer, Synthesizer(equalizer=)) against the serial float64 recurrence
(tests/equalizer_reference.py), and bit for bit where the contract says so.

Bound, per item:  |out - y64| <= 2^-23 * P,  P the largest magnitude among the item's input and every section's float64 output.
2^-24 P is the one fp32 rounding of the output (|y_N| <= P).  The same again is room for what float64 does differently in the
kernel: it adds the contributions of earlier chunks and segments to a state in another order than the serial recurrence, and
uses fma where numpy rounds twice.  Each such difference is a rounding of 2^-53 of a state, amplified by at most the largest
power of a section's transition (below 1 / (1 - |pole|) = 2,200 for the 5 Hz corner used here) over some thousand steps:
around 1e-10 P, three orders below the room.  The tests print the worst ratio; DESIGN.md 4.28 records it.
Measured on an MI355X over the cases below: worst |out - y64| 0.401 of the bound at N = 1, 0.338 at N = 2, 0.245 at N = 8 - under
0.5, the fp32 rounding and nothing else (test_against_float64 prints the figures)."""
import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

import equalizer_reference as R
from isp_tts_amd import graph, longform, runtime, synth
from isp_tts_amd.data import (AudioConditioner, Equalizer, highpass, highshelf, lowpass, lowshelf, notch, peaking, preemphasis)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEG = runtime.EQ_SEGMENT_SAMPLES
S, LD = 3 * SEG + 77, 3 * SEG + 84                                          # a row stride above S (a multiple of four floats)
ROW_LENS = [0, 1, 31, 32, 33, SEG - 1, SEG, SEG + 1, 2 * SEG, S, -1, S + 1]
B = len(ROW_LENS)
RATE = 48000
BOUND = 2.0 ** -23


def bits(t):
    return t.detach().cpu().numpy().tobytes()


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


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


def cascade(n):
    """Moderate gains (within +-12 dB); the 5 Hz and 20 Hz corners carry state over many segments."""
    return {1: [highpass(20.0)], 2: [highpass(5.0), peaking(1000.0, 6.0, 2.0)],
            8: [highpass(5.0), highpass(20.0), lowshelf(150.0, 4.0), peaking(1000.0, 6.0, 2.0), notch(50.0, 10.0),
                peaking(3000.0, -5.0), highshelf(8000.0, -3.0), lowpass(0.45 * RATE)]}[n]


_CASE = {}


def case():
    """The batch, made once: noise plus a DC offset of 0.5, NaN wherever the kernel has no business reading."""
    if not _CASE:
        clean = (0.25 * np.random.default_rng(1).standard_normal((B, S)) + 0.5).astype(np.float32)
        lens = np.array(ROW_LENS, np.int64)
        audio = np.full((B, LD), np.nan, np.float32)
        for b, n in enumerate(R.kept(lens, S)):
            audio[b, :n] = clean[b, :n]
        _CASE.update(clean=clean, lens=lens, audio_d=dev(audio)[:, :S], lens_d=dev(lens), refs={})
        assert _CASE["audio_d"].stride(0) == LD
    return _CASE


def reference(key, sos):
    c = case()
    if key not in c["refs"]:
        c["refs"][key] = R.equalize_ref(c["clean"], c["lens"], sos)
    return c["refs"][key]


def run(eq, audio, lens, out=None, out_len=None):
    r = runtime.equalize(audio, lens, eq.device_tables(DEV), eq.sections, out, out_len)
    torch.cuda.synchronize()
    return r


# ------------------------------------------------------------------------------------------------ against float64
@pytest.mark.parametrize("n", [1, 2, 8])
def test_against_float64(n):
    c = case()
    eq = Equalizer(RATE, cascade(n))
    ref, ref_len, P = reference(n, eq.sos)
    full = torch.full((B, LD), 7.0, device=DEV)
    out, out_len = run(eq, c["audio_d"], c["lens_d"], out=full[:, :S])
    got = host(out)
    assert np.array_equal(host(out_len), ref_len)
    assert bits(full[:, S:]) == bits(torch.full((B, LD - S), 7.0))             # nothing behind column S is written
    assert np.isfinite(got).all()                                              # no NaN: nothing at or past a length was read
    worst, flips, total = 0.0, 0, 0
    for b in range(B):
        m = int(ref_len[b])
        assert not got[b, m:].any(), b                                         # exactly zero from the length on
        if m == 0:
            continue
        # (where the kernel's float64 and the reference's round to different fp32 values: a measure of how far the two are apart)
        flips, total = flips + int((got[b, :m] != ref[b, :m].astype(np.float32)).sum()), total + m
        err = float(np.abs(got[b, :m] - ref[b, :m]).max())
        worst = max(worst, err / (BOUND * P[b]))
        print(f"N={n} row {b} len {m}: |out - y64| {err:.3e} = {err / (BOUND * P[b]):.3f} of the bound (P {P[b]:.3f})")
        assert err <= BOUND * P[b], (n, b, err, BOUND * P[b])
    print(f"N={n}: worst |out - y64| {worst:.3f} of the bound; {flips} of {total} samples are not fp32(y64)")


def test_carry_across_segments():
    """A 20 Hz and a 5 Hz high-pass at 48 kHz (pole radii 0.99815 and 0.99954): first that the test can tell - a reference that
    drops the carry misses by far more than 100 bounds - then the kernel."""
    c = case()
    b = ROW_LENS.index(S)
    x = c["clean"][b:b + 1].astype(np.float64)
    for f0 in (20.0, 5.0):
        eq = Equalizer(RATE, [highpass(f0)])
        ref, _, P = R.equalize_ref(c["clean"][b:b + 1], [S], eq.sos)
        bound = BOUND * P[0]
        reset = float(np.abs(R.reset_at_borders(x, eq.sos) - ref).max()) / bound
        short = float(np.abs(R.one_segment_memory(x, eq.sos) - ref).max()) / bound
        print(f"{f0} Hz: a reference that resets at segment borders misses by {reset:.3g} bounds, one that forgets what is older "
              f"than a segment by {short:.3g}")
        assert reset > 100.0
        if f0 == 5.0:
            assert short > 100.0
        out, _ = run(eq, c["audio_d"][b:b + 1], c["lens_d"][b:b + 1])
        err = float(np.abs(host(out)[0] - ref[0]).max()) / bound
        print(f"{f0} Hz: the kernel, {err:.3f} of the bound")
        assert err <= 1.0


def test_fir_sections_are_bit_exact():
    """The lane matrices of a section without poles are nilpotent - zero from the second power on - so the scan adds nothing: fp32
    of the serial float64 recurrence, bit for bit.  (Exact in numpy as well: with b0 = 1 and b2 = 0 every product but one is
    exact, so fma and two roundings agree.)"""
    c = case()
    for bands in ([preemphasis()], [preemphasis(), preemphasis()]):
        eq = Equalizer(RATE, bands)
        ref, ref_len, _ = R.equalize_ref(c["clean"], c["lens"], eq.sos)
        out, out_len = run(eq, c["audio_d"], c["lens_d"])
        assert np.array_equal(host(out_len), ref_len)
        assert bits(out) == ref.astype(np.float32).tobytes(), len(bands)


def test_identity_section():
    c = case()
    eq = Equalizer(RATE, sos=[[1.0, 0.0, 0.0, 0.0, 0.0]])
    out, out_len = run(eq, c["audio_d"], c["lens_d"])
    want = np.where(np.arange(S)[None, :] < R.kept(c["lens"], S)[:, None], c["clean"], np.float32(0.0))
    assert bits(out) == want.tobytes() and np.array_equal(host(out_len), R.kept(c["lens"], S))


# ------------------------------------------------------------------------------------------------ bit for bit
def test_batch_alignment_in_place():
    c = case()
    eq = Equalizer(RATE, cascade(8))
    out, out_len = run(eq, c["audio_d"], c["lens_d"])
    again = run(eq, c["audio_d"], c["lens_d"])
    assert bits(again[0]) == bits(out) and bits(again[1]) == bits(out_len)
    # an item alone
    for b in (2, 5, 7, 9):
        o1, n1 = run(eq, c["audio_d"][b:b + 1], c["lens_d"][b:b + 1])
        assert bits(o1[0]) == bits(out[b]) and int(n1[0]) == int(out_len[b]), b
    # a view offset by one float, input and output: no 16-byte access anywhere
    shifted = torch.full((B, LD + 1), float("nan"), device=DEV)
    shifted[:, 1:] = c["audio_d"].as_strided((B, LD), (LD, 1))
    full = torch.full((B, LD + 1), 7.0, device=DEV)
    o2, n2 = run(eq, shifted[:, 1:1 + S], c["lens_d"], out=full[:, 1:1 + S])
    assert o2.data_ptr() % 16 == 4 and bits(o2) == bits(out) and bits(n2) == bits(out_len)
    assert bits(full[:, :1]) == bits(torch.full((B, 1), 7.0)) and bits(full[:, 1 + S:]) == bits(torch.full((B, LD - S), 7.0))
    # in place: out is audio, same base and row stride
    buf = c["audio_d"].as_strided((B, LD), (LD, 1)).clone()
    o3, n3 = run(eq, buf[:, :S], c["lens_d"], out=buf[:, :S])
    assert o3.data_ptr() == buf.data_ptr() and bits(o3) == bits(out) and bits(n3) == bits(out_len)
    assert torch.isnan(buf[:, S:]).all()                                       # the padding of the rows is as it was
    # any other overlap is refused
    with pytest.raises(runtime.IspkError, match="overlaps"):
        runtime.equalize(buf[:, :S], c["lens_d"], eq.device_tables(DEV), 8, out=buf.view(-1)[1:].as_strided((B, S), (LD, 1)))
    with pytest.raises(runtime.IspkError, match="overlaps"):
        runtime.equalize(buf[:4, :S], c["lens_d"][:4], eq.device_tables(DEV), 8, out=buf[3:7, :S])


def test_sine_through_a_peak():
    """1 kHz through peaking(1000, +6 dB, q = 1) at 22,050 Hz: past the transient the RMS gain is |H(1000)|.  Over 37 * 441 samples
    (740 whole periods) both RMS values are exact up to the fp32 roundings of the samples, 6e-8 each and averaged."""
    rate = 22050
    eq = Equalizer(rate, [peaking(1000.0, 6.0, 1.0)])
    n = SEG + 37 * 441
    x = (0.5 * np.sin(2.0 * np.pi * 1000.0 * np.arange(n) / rate)).astype(np.float32)
    out, _ = run(eq, dev(x[None, :]), dev([n], np.int64))
    y = host(out)[0].astype(np.float64)
    gain = np.sqrt(np.mean(y[SEG:] ** 2) / np.mean(x[SEG:].astype(np.float64) ** 2))
    want = float(np.abs(eq.response([1000.0]))[0])
    print(f"RMS gain {gain:.9f}, |H(1000)| {want:.9f}")
    assert abs(want - 10.0 ** (6.0 / 20.0)) <= 1e-12 and abs(gain - want) <= 1e-6


# ------------------------------------------------------------------------------------------------ no ATen op, graph capture
def test_no_aten_op_and_graph_replay():
    c = case()
    eq = Equalizer(RATE, cascade(8))
    eager, eager_len = run(eq, c["audio_d"], c["lens_d"])
    out = eq.empty_outputs(B, S, DEV)
    eq.device_tables(DEV)
    spy = Spy()
    with spy:
        r = eq(c["audio_d"], c["lens_d"], out=out)
    torch.cuda.synchronize()
    assert spy.seen == [], spy.seen
    assert set(r) == {"audio", "audio_len"} and r["audio"] is out["audio"] and r["audio_len"] is out["audio_len"]
    assert bits(r["audio"]) == bits(eager) and bits(r["audio_len"]) == bits(eager_len)
    static = eq.empty_outputs(B, S, DEV)
    g = graph.GraphedCall(lambda: eq(c["audio_d"], c["lens_d"], out=static))
    static["audio"].fill_(3.0)
    static["audio_len"].fill_(-5)
    torch.cuda.synchronize()
    spy = Spy()
    with spy:
        r = g.replay()
    torch.cuda.synchronize()
    assert spy.seen == [], spy.seen
    assert bits(r["audio"]) == bits(eager) and bits(r["audio_len"]) == bits(eager_len)


# ------------------------------------------------------------------------------------------------ the Synthesizer
B_S, L_S, M_S, D_S = 4, 16, 128, 2


@pytest.fixture(scope="module")
def hifigan():
    from isp_tts_amd.hifigan import HifiGan
    return HifiGan.from_state_dict(synth.make_hifigan_state_dict(), synth.HIFIGAN_DIMS["v1"]).to(DEV).eval()


def test_synthesizer_with_equalizer(gpu_model, hifigan):
    S_out, rate = 70000, 22050
    kw = dict(batch=B_S, tokens=L_S, frames=M_S, docs=D_S, doc_samples=S_out, steps=4, fade=64)
    inp = synth.make_inputs(B_S, L_S, M_S, variable=False, seed=44)
    noise = inp["flow_x0"].to(DEV).clone()
    noise[..., 0] += 1.0                                                       # longer items
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=DEV)             # noqa: E731
    text, tl, doc, pos, pause = inp["text"].to(DEV), inp["text_len"].to(DEV), i64([0, 1, 0, 1]), i64([0, 0, 1, 1]), i64([500, 0, 0, 0])
    controls = longform.make_controls(B_S, duration_factor=8.0, device=DEV)

    def call(syn):
        r = syn(text, tl, doc, pos, pause, controls, flow_noise=noise)
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in r.items() if v is not None}

    # equalizer=None: the bits of a Synthesizer built without the argument
    cond = AudioConditioner(rate)
    without = call(longform.Synthesizer(gpu_model, hifigan, item_conditioner=cond, **kw))
    none = call(longform.Synthesizer(gpu_model, hifigan, item_conditioner=cond, equalizer=None, **kw))
    assert set(none) == set(without)
    for k in without:
        assert bits(none[k]) == bits(without[k]), k
    # with one: the stages by hand over the vocoder's audio
    eq = Equalizer(rate, [highpass(80.0)])
    syn = longform.Synthesizer(gpu_model, hifigan, item_conditioner=cond, equalizer=eq, **kw)
    got = call(syn)
    assert set(got) == set(without)
    wav, wav_len = syn._wav[0].clone(), syn._wav[1].clone()
    print(f"item lengths {wav_len.tolist()} of {wav.shape[1]} samples")
    assert int(wav_len.max()) > SEG                                            # an item of more than one segment
    heard = eq(wav, wav_len)
    bounds, _, _, gain = runtime.audio_measure(heard["audio"], wav_len, cond.device_tables(DEV), rate, cond.trim_mode, cond.trim_threshold,
                                               cond.pad_frames, 1, cond.target_lufs, cond.peak_limit)
    j = longform.join(heard["audio"], wav_len, doc, pos, pause, num_docs=D_S, out_samples=S_out, bounds=bounds, gain=gain, fade=64)
    torch.cuda.synchronize()
    assert bits(j["audio"]) == bits(got["audio"]) and bits(j["audio_len"]) == bits(got["audio_len"])
    assert bits(got["audio"]) != bits(without["audio"])                        # the stage is in the chain
    longest = int(wav_len.argmax())
    ref, _, P = R.equalize_ref(host(wav)[longest:longest + 1], host(wav_len)[longest:longest + 1], eq.sos)
    assert np.abs(host(heard["audio"])[longest] - ref[0]).max() <= BOUND * P[0]
    with pytest.raises(ValueError, match="equalizer"):
        longform.Synthesizer(gpu_model, hifigan, equalizer="bright", **kw)
