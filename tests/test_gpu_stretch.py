"""GPU: the time stretch (data.TimeStretch: csrc/stretch.hip, ispk_stretch_f32) and data.PitchShift against the float64
restatement of tests/stretch_reference.py, which is written in the textbook form (angles, w_k, wrap) while the kernels multiply
unit phasors: the tests also prove the two equal.

Inputs (stretch_reference.signal): seeded white noise of 0.1, or noise of 0.05 plus a gliding 7-harmonic tone - broadband, because
a pure tone is ill-conditioned (the phase of its empty bins is rounding noise that accumulates); tones appear in the property
tests only.  Lengths 0, 512, 513, 1024, 4095, 4096, 4097, 8191, 12288 (the short boundary, the edges of the analysis tiles, 97
output frames = seven chunks of the scan and six output tiles at rate 0.5) at the rates 0.5, 0.8, 1.0, 1.25, 1.37, 2.0, in
ragged batches of at most 5; padded row strides, NaN behind n, a sentinel behind out_samples.

Bound.  Not fixed in advance: per item e_mixed = the error of the mixed chain (torch's fp32 stft on the CPU, float64 phases modulo
2 pi, fp32 inverse) against the reference, over the reference's peak; the kernel must lie within 8 x e_mixed (this project's margin
for "a different fp32 FFT than torch's", tests/test_gpu_screen.py, tests/test_gpu_noise.py), and 8 x e_mixed <= 2e-4 is asserted so
that a degenerate input cannot loosen the test.  out_len, wanted and flags with ==.
Measured on gfx950: errors of 1.3e-7 .. 7.6e-6 of the peak where e_mixed is 1.3e-7 .. 6.7e-6; at worst 0.214 of the bound on the
grid (n = 12288 at rate 2.0) and 0.378 over the whole file (n = 5119 at rate 0.5 under truncation: 2.27e-6 against 7.5e-7).

Then the integers under truncation, rate 1 against the input itself, per-item device rates = the scalar entry bit for bit (row
stride, padding, B, S, out_samples), NaN and out-of-range device rates, repeated calls and a graph replay, TimeStretch ->
AudioConditioner -> to_pcm16 as one HIP graph without ATen compute, and the properties of a tone under stretch and pitch shift."""
import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

import stretch_reference as R
from isp_tts_amd import graph, runtime
from isp_tts_amd.data import AudioConditioner, PitchShift, Resampler, TimeStretch, to_pcm16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TS = runtime.STRETCH_TILE_SAMPLES
RATES = (0.5, 0.8, 1.0, 1.25, 1.37, 2.0)
LENGTHS = (0, 512, 513, 1024, 4095, 4096, 4097, 8191, 12288)
BATCHES = {"a": (0, 513, 4095, 4097, 12288), "b": (512, 1024, 4096, 8191)}
assert sorted(n for b in BATCHES.values() for n in b) == sorted(LENGTHS) and TS == 4096
MARGIN, CEILING = 8.0, 2e-4
SENTINEL = 7.0
_CACHE = {}


class Spy(TorchDispatchMode):
    """Records every ATen op that touches a GPU tensor, views and allocations apart (tests/test_gpu_noise.py's)."""
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


def bits(t):
    return t.detach().cpu().numpy().tobytes()


def host(t):
    return t.detach().cpu().numpy()


def signal(n, r):
    return R.signal(n, 100 * n + RATES.index(r) if r in RATES else 100 * n + 7)


def reference(n, r):
    """(x, the float64 output, e_mixed) for signal(n, r), made once."""
    key = (n, r)
    if key not in _CACHE:
        x = signal(n, r)
        want = R.stretch_item(x, r)
        e = R.relative_error(R.mixed_item(x, r), want)
        assert 0.0 < MARGIN * e <= CEILING, f"n={n} r={r}: 8 x e_mixed = {MARGIN * e:.2e} is no bound"
        _CACHE[key] = (x, want, e)
    return _CACHE[key]


def run(ts, xs, lens, rate, S, out_samples, pad_in=5, pad_out=3, fill=float("nan"), use_len=None):
    """xs: the items (float64); the rest of each row is `fill`, never to be read.  rate: a float or a list (a device tensor is
    made of it) -> the call's dict on the CPU, "audio" [B, out_samples]."""
    B = len(xs)
    a = torch.full((B, S + pad_in), fill, dtype=torch.float32)
    for b, x in enumerate(xs):
        a[b, :len(x)] = torch.from_numpy(x).float()
    o = torch.full((B, out_samples + pad_out), SENTINEL, device=DEV)
    ln = torch.tensor(lens if use_len is None else use_len, dtype=torch.int64, device=DEV)
    if not isinstance(rate, float):
        rate = torch.tensor(rate, dtype=torch.float64, device=DEV)
    r = ts(a.to(DEV)[:, :S], ln, rate=rate, out={"audio": o[:, :out_samples]})
    torch.cuda.synchronize()
    assert set(r) == {"audio", "audio_len", "wanted", "flags"} and r["audio"].data_ptr() == o.data_ptr()
    assert r["audio_len"].dtype == r["wanted"].dtype == torch.int64 and r["flags"].dtype == torch.int32
    assert (o[:, out_samples:] == SENTINEL).all(), "columns past out_samples were written"
    return {k: v.cpu() for k, v in r.items()}


def check_integers(r, lens, rates, out_samples, what):
    for b, n in enumerate(lens):
        want = R.lengths(n, rates[b], out_samples)
        got = (int(r["audio_len"][b]), int(r["wanted"][b]), int(r["flags"][b]))
        assert got == want, f"{what} n={n} r={rates[b]}: (out_len, wanted, flags) = {got}, the reference has {want}"


def check_item(got, out_len, x, r, what):
    """One row against float64 within 8 x e_mixed below out_len, exact zeros behind; a bit copy below 513 samples -> error / bound."""
    n = len(x)
    assert (got[out_len:] == 0).all(), f"{what}: non-zero samples at or past out_len"
    if n < R.MIN_SAMPLES:
        assert torch.equal(got[:out_len], torch.from_numpy(x).float()[:out_len]), f"{what}: a short item is copied bit for bit"
        return 0.0
    _, want, e = reference(n, r)
    err = np.abs(got[:out_len].double().numpy() - want[:out_len])
    peak = float(np.abs(want).max())
    rel = float(err.max()) / peak
    print(f"{what}: max |err| / peak = {rel:.3e}, e_mixed = {e:.3e}, of the bound {rel / (MARGIN * e):.3f}")
    for s in (TS - 1, TS, TS + 1, 2 * TS - 1, 2 * TS, 2 * TS + 1):             # the output tiles' edges, explicitly
        if s < out_len:
            assert err[s] <= MARGIN * e * peak, f"{what}: sample {s} at an output tile edge is off by {err[s]:.3e}"
    assert rel <= MARGIN * e, f"{what}: max |err| / peak {rel:.3e} > 8 x e_mixed = {MARGIN * e:.3e}"
    return rel / (MARGIN * e)


# ------------------------------------------------------------------------------------------------ against float64
@pytest.mark.parametrize("name", list(BATCHES))
@pytest.mark.parametrize("rate", RATES)
def test_against_float64(rate, name):
    assert runtime.lib().ispk_stretch_tile_samples() == TS
    lens = BATCHES[name]
    S = max(lens) + 37
    xs = [signal(n, rate) for n in lens]
    out_samples = TimeStretch.out_samples(S, rate)
    r = run(TimeStretch(rate), xs, lens, rate, S, out_samples)
    check_integers(r, lens, [rate] * len(lens), out_samples, f"batch {name}")
    assert not (host(r["flags"]) & R.TRUNCATED).any()
    worst = max(check_item(r["audio"][b], int(r["audio_len"][b]), xs[b], rate, f"batch {name} r={rate} n={n}") for b, n in enumerate(lens))
    print(f"stretch batch {name} {lens} at {rate}: worst error / (8 x e_mixed) = {worst:.3f}")


@pytest.mark.parametrize("rate", (0.5, 1.25))
def test_integers_and_audio_under_truncation(rate):
    lens = (513, 4096, 5119, 12288, 0)
    S, out_samples = 12288, 4100                                               # cuts the long items inside their second output tile
    xs = [signal(n, rate) for n in lens]
    r = run(TimeStretch(), xs, lens, rate, S, out_samples)
    check_integers(r, lens, [rate] * len(lens), out_samples, "truncated")
    assert R.plan(5119, 1.25)[:2] == (20, 16)                                  # F / r an exact integer
    flags = host(r["flags"])
    assert (flags[3] & R.TRUNCATED) and flags[4] == R.SHORT and int(r["audio_len"][3]) == out_samples
    for b, n in enumerate(lens):
        check_item(r["audio"][b], int(r["audio_len"][b]), xs[b], rate, f"truncated r={rate} n={n}")


def test_rate_one_returns_the_input():
    """No reference involved: the bound is 8 x the mixed chain's error against the input itself."""
    lens = (513, 4097, 12288)
    xs = [R.signal(n, n) for n in lens]
    r = run(TimeStretch(1.0), xs, lens, 1.0, 12288, 12289)
    for b, n in enumerate(lens):
        assert int(r["audio_len"][b]) == int(r["wanted"][b]) == n and int(r["flags"][b]) == 0
        e = R.relative_error(R.mixed_item(xs[b], 1.0), xs[b])
        assert 0.0 < MARGIN * e <= CEILING
        rel = R.relative_error(r["audio"][b, :n].double().numpy(), xs[b])
        print(f"rate 1, n={n}: max |err| / peak = {rel:.3e}, e_mixed = {e:.3e}, of the bound {rel / (MARGIN * e):.3f}")
        assert rel <= MARGIN * e and (r["audio"][b, n:] == 0).all()


# ------------------------------------------------------------------------------------------------ bit identity
def test_per_item_rates_equal_the_scalar_entry():
    lens = (4097, 12288, 1024, 8191, 513, 6000)
    rates = [0.5, 0.8, 1.25, 1.37, 2.0, 1.0]
    S, out_samples = 12288, 2 * 12288 + 1
    xs = [signal(n, rate) for n, rate in zip(lens, rates)]
    ts = TimeStretch()
    base = run(ts, xs, lens, rates, S, out_samples)
    check_integers(base, lens, rates, out_samples, "per item")
    for b, (n, rate) in enumerate(zip(lens, rates)):
        wanted = round(n / rate)
        # alone, through the scalar entry: another B, S, row stride and out_samples (exactly wanted), zeros behind n
        alone = run(ts, [xs[b]], [n], float(rate), n, wanted, pad_in=2, pad_out=1, fill=0.0)
        assert int(alone["audio_len"][0]) == wanted == int(base["audio_len"][b]) and int(alone["flags"][0]) == 0
        assert torch.equal(alone["audio"][0], base["audio"][b, :wanted]), f"n={n} r={rate}: the batch changed an item's bits"
        assert (base["audio"][b, wanted:] == 0).all()
        if rate in RATES:
            check_item(base["audio"][b], wanted, xs[b], rate, f"per item r={rate} n={n}")
    for fill in (0.0, 1e30):                                                   # base ran with NaN behind the lengths
        assert bits(run(ts, xs, lens, rates, S, out_samples, fill=fill)["audio"]) == bits(base["audio"]), fill
    other = run(ts, xs, lens, rates, S + 41, out_samples + 300, pad_in=8, pad_out=6)               # S, out_samples and the strides
    assert torch.equal(other["audio"][:, :out_samples], base["audio"]) and (other["audio"][:, out_samples:] == 0).all()
    sub = run(ts, xs[1:4], lens[1:4], rates[1:4], S, out_samples)              # another B
    assert torch.equal(sub["audio"], base["audio"][1:4])


def test_bad_device_rates_and_lengths_are_copied():
    lens = (4097, 1024, 2000, 3000, 1024)
    rates = [float("nan"), 3.0, 0.4999, 1.25, 2.0]
    xs = [R.signal(n, n) for n in lens]
    S, out_samples = 4200, 4200
    r = run(TimeStretch(), xs, lens, rates, S, out_samples, use_len=(4097, 1024, 2000, 3000, S + 1))
    assert host(r["flags"]).tolist() == [R.BAD_RATE, R.BAD_RATE, R.BAD_RATE, 0, R.SHORT]
    assert host(r["audio_len"]).tolist() == [4097, 1024, 2000, 2400, 0] == host(r["wanted"]).tolist()
    for b in range(3):
        assert torch.equal(r["audio"][b, :lens[b]], torch.from_numpy(xs[b]).float()) and (r["audio"][b, lens[b]:] == 0).all(), b
    assert (r["audio"][4] == 0).all() and not torch.equal(r["audio"][3, :2400], torch.from_numpy(xs[3]).float()[:2400])
    cut = run(TimeStretch(), xs[:1], lens[:1], [3.0], S, 1000)                 # a copy, truncated
    assert host(cut["flags"]).tolist() == [R.BAD_RATE | R.TRUNCATED] and int(cut["audio_len"][0]) == 1000 and int(cut["wanted"][0]) == 4097
    assert torch.equal(cut["audio"][0], torch.from_numpy(xs[0]).float()[:1000])


def test_repeats_and_graph_replay():
    lens = (12288, 4097, 513, 100)
    rates = torch.tensor([0.8, 1.25, 2.0, 1.0], dtype=torch.float64, device=DEV)
    S, out_samples = 12288, 16000
    audio = torch.zeros((len(lens), S))
    for b, n in enumerate(lens):
        audio[b, :n] = torch.from_numpy(R.signal(n, n)).float()
    audio, ln = audio.to(DEV), torch.tensor(lens, dtype=torch.int64, device=DEV)
    ts = TimeStretch()
    eager = {k: v.clone() for k, v in ts(audio, ln, rate=rates, out_samples=out_samples).items()}
    again = ts(audio, ln, rate=rates, out_samples=out_samples)
    torch.cuda.synchronize()
    for k in eager:
        assert bits(again[k]) == bits(eager[k]), k
    static = ts.empty_outputs(len(lens), DEV, samples=out_samples)
    spy = Spy()
    with spy:
        r = ts(audio, ln, rate=rates, out=static)
    torch.cuda.synchronize()
    assert spy.seen == [], spy.seen
    assert all(r[k] is static[k] for k in eager)
    g = graph.GraphedCall(lambda: ts(audio, ln, rate=rates, out=static))
    for _ in range(2):
        for k in eager:
            static[k].fill_(3)
        torch.cuda.synchronize()
        r = g.replay()
        torch.cuda.synchronize()
        for k in eager:
            assert bits(r[k]) == bits(eager[k]), k
    rates.copy_(torch.tensor([1.25, 1.25, 0.5, 7.0], dtype=torch.float64))     # one capture serves every draw
    r = g.replay()
    torch.cuda.synchronize()
    assert host(r["audio_len"]).tolist() == [9830, 3278, 1026, 100] and host(r["flags"]).tolist() == [0, 0, 0, R.SHORT | R.BAD_RATE]
    assert bits(r["audio"][1]) == bits(eager["audio"][1])


def test_stretch_condition_pcm16_as_one_graph():
    lens = (12288, 6000)
    S, rate = 12288, 1.25
    out_samples = TimeStretch.out_samples(S, rate)
    audio = torch.zeros((2, S))
    for b, n in enumerate(lens):
        audio[b, :n] = torch.from_numpy(R.glide_signal(n, 11 + b)).float()
    audio, ln = audio.to(DEV), torch.tensor(lens, dtype=torch.int64, device=DEV)
    ts, cond = TimeStretch(rate), AudioConditioner(R.RATE_HZ, top_db=None)
    ts.device_tables(DEV), cond.device_tables(DEV)

    def chain(st, co, pcm):
        s = ts(audio, ln, out=st)
        c = cond(s["audio"], s["audio_len"], out=co)
        return to_pcm16(c["audio"], c["audio_len"], out=pcm), c["audio_len"]

    new = lambda: (ts.empty_outputs(2, DEV, samples=out_samples), cond.empty_outputs(2, out_samples, DEV),      # noqa: E731
                   torch.empty((2, out_samples), dtype=torch.int16, device=DEV))
    pcm, n = chain(*new())
    torch.cuda.synchronize()
    eager = (pcm.clone(), n.clone())
    assert host(n).tolist() == [round(12288 / rate), round(6000 / rate)] and int(eager[0].abs().max()) > 1000
    static = new()
    g = graph.GraphedCall(lambda: chain(*static))
    for _ in range(2):
        static[2].fill_(3)
        spy = Spy()
        with spy:
            pcm, n = g.replay()
        torch.cuda.synchronize()
        assert spy.seen == [], spy.seen
        assert bits(pcm) == bits(eager[0]) and bits(n) == bits(eager[1])


# ------------------------------------------------------------------------------------------------ properties
def tone_batch(n=12288):
    x = R.tone_signal(n, 5)
    return x, torch.from_numpy(x).float()[None].to(DEV), torch.tensor([n], dtype=torch.int64, device=DEV)


@pytest.mark.parametrize("rate", (0.8, 1.25))
def test_stretched_tone_keeps_its_peak(rate):
    x, audio, ln = tone_batch()
    r = TimeStretch(rate)(audio, ln)
    torch.cuda.synchronize()
    n_out = int(r["audio_len"][0])
    assert n_out == int(r["wanted"][0]) == round(len(x) / rate) and int(r["flags"][0]) == 0
    y = host(r["audio"][0, :n_out]).astype(np.float64)
    assert R.peak_bin(y) == R.peak_bin(x) == round(440.0 * 8192 / R.RATE_HZ)


def test_pitch_shift_moves_the_peak_and_keeps_the_length():
    x, audio, ln = tone_batch()
    ps = PitchShift(R.RATE_HZ, ratio=(5, 4))
    r = ps(audio, ln)
    torch.cuda.synchronize()
    n_out = int(r["audio_len"][0])
    assert abs(n_out - len(x)) <= 1 and n_out == -(-4 * round(len(x) * 5 / 4) // 5)
    y = host(r["audio"][0, :n_out]).astype(np.float64)
    assert abs(R.peak_bin(y) - 550.0 * 8192 / R.RATE_HZ) <= 1.0 and R.peak_bin(x) == 163
    # the two stages by hand
    s = TimeStretch(4 / 5)(audio, ln, out_samples=ps.stretched_samples(len(x)))
    a, n = Resampler(5, 4)(s["audio"], s["audio_len"])
    torch.cuda.synchronize()
    assert bits(a) == bits(r["audio"]) and bits(n) == bits(r["audio_len"]) and bits(s["audio"]) == bits(r["stretched"])
    out = ps.empty_outputs(1, len(x), DEV)                                     # preallocated: the pair captures
    spy = Spy()
    with spy:
        again = ps(audio, ln, out=out)
    torch.cuda.synchronize()
    assert spy.seen == [] and again["audio"] is out["audio"] and bits(again["audio"]) == bits(r["audio"])
