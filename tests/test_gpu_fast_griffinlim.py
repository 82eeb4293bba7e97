"""GPU: the fast (momentum) Griffin-Lim iteration (isp_tts_amd.griffinlim.FastGriffinLim: one launch of
ispk_griffinlim_fast_step_f32 per iteration from the second on) against the float64 textbook reference of
tests/fast_griffinlim_reference.py, which keeps the complex tprev, and the on-device spectral convergence
(GriffinLim.spectral_convergence: ispk_griffinlim_error_f32) against float64 on the host.

Inputs, frame counts and batches are tests/test_gpu_griffinlim.py's: synth.make_clip at amplitude 0.5 cut to n = 256 T samples,
T in 0, 1, 2, 3, 4 (fewer frames than the four that overlap), 15, 16, 17 (the 16-hop tile edge and the error kernel's 16-frame
block edge), 32, 33 (a second and third tile), each alone and inside the two ragged batches of five whose padded T exceeds the
longest item, with padded row strides, NaN past the lengths and sentinel columns in `out`.

Bounds: after 1, 2 and 4 iterations at momentum 0.99 and 0.5, max |err| <= 1e-4 x the item's peak against the textbook
reference (torch's fp32 chain on the CPU: 8e-7, 1.5e-6, 3.1e-6).  From the second iteration on the plain and the fast reference
differ by at least 0.02 of the peak on these items (asserted at 0.01), so the bound also proves that the momentum is applied.  A
full run is held to its spectral convergence, computed on the host in float64 after 1, 2, 4, 8, 16 and 32 iterations, each
from scratch: within a relative 1e-3 of the textbook reference's (fp32 on the CPU: 2.0e-5; the trajectories differ by up to
7.4e-4 of the peak at 32), and at 32 iterations at most 0.75 x that of the plain GPU run from the same start.  The device's
spectral convergence of a GPU iterate is within a relative 1e-5 of the host's float64 figure for the same waveform where that
is at least 0.01 (fp32 on the CPU: 1.2e-7), and at most 1e-5 for a clip with its own magnitude (1e-7).

Measured on gfx950 (worst over the items alone and in the batches, both momenta):
    one iteration                         max |err| / peak 4.5e-7
    two iterations                        max |err| / peak 8.3e-7
    four iterations                       max |err| / peak 3.0e-6
    spectral convergence, 6 counts        relative difference to float64 at most 1.2e-6 harmonic, 5.5e-6 chirp, 9.6e-7 noise
    at 32 iterations over the plain run   harmonic 0.268, chirp 0.438, noise 0.604
    device spectral convergence           relative difference to float64 at most 1.2e-7; own magnitude at most 1.0e-7

Then bit identity (n_iter 0 and 1 and momentum 0 against the plain path, ragged batch = alone, padding contents, lengths out of
range, repeated calls, seeds, every n_iter landing in `out` eagerly and as a replayed graph), the whole text -> PCM16 chain as
one graph, and the absence of ATen compute."""
import numpy as np
import pytest
import torch

import fast_griffinlim_reference as fr
import griffinlim_reference as gr
from isp_tts_amd import graph, synth
from isp_tts_amd.griffinlim import FastGriffinLim, GriffinLim
from test_gpu_griffinlim import BATCHES, DEV, FRAMES, FULL_RUN, KINDS, SENTINEL, _acoustic_model, _audio_batch, _mag_batch

pytestmark = pytest.mark.gpu
FP32_REL = 1e-4
MOMENTA = (0.99, 0.5)
STEPS = (1, 2, 4)
COUNTS = (1, 2, 4, 8, 16, 32)


@pytest.fixture(scope="module")
def gl():
    return FastGriffinLim(n_iter=32, seed=0).to(DEV)


@pytest.fixture(scope="module")
def plain():
    return GriffinLim(n_iter=32, seed=0).to(DEV)


@pytest.fixture(scope="module")
def items():
    """T -> the item's clip, its float64 magnitude rounded to fp32, the plain float64 waveforms after 0, 1, 2 and 4 iterations
    and, per momentum, the textbook fast ones after 1, 2 and 4, from the hashed phase of seed 0; made once, never changed."""
    cache = {}

    def get(T):
        if T not in cache:
            x = synth.make_clip(KINDS[T % len(KINDS)], 256 * T, 0.5).double().numpy()
            M = np.abs(gr.stft(x)).astype(np.float32).astype(np.float64)
            cache[T] = dict(x=x, M=M, plain=gr.griffinlim(M, 4, seed=0, keep=(0, 1, 2, 4)),
                            fast={m: fr.textbook(M, 4, m, seed=0, keep=STEPS) for m in MOMENTA})
        return cache[T]
    return get


def _iterate(gl, mags, lens, Tp, n_iter, seed=0, init=None, fill=float("nan"), **kw):
    """-> (audio [B, 256 Tp] on the CPU, audio_len [B]); checks the sentinel columns and the returned objects."""
    B, S = len(mags), 256 * Tp
    o = torch.full((B, S + 3), SENTINEL, device=DEV)
    ol = torch.full((B,), -5, dtype=torch.int64, device=DEV)
    ln = torch.tensor(lens, dtype=torch.int64, device=DEV)
    a = None if init is None else _audio_batch(init, Tp, fill)
    got, got_len = gl.from_magnitude(_mag_batch(mags, Tp, fill), ln, init=a, n_iter=n_iter, seed=seed, out=(o[:, :S], ol), **kw)
    torch.cuda.synchronize()
    assert got.data_ptr() == o.data_ptr() and got_len is ol
    assert (o[:, S:] == SENTINEL).all(), "columns past 256 T were written"
    return o[:, :S].cpu(), ol.cpu()


def _check_item(got, want, what):
    """One utterance's row against float64: the bound below n, exact zeros from n on."""
    n = len(want)
    assert (got[n:] == 0).all(), f"{what}: non-zero samples at or past n"
    if n == 0:
        return 0.0
    peak = float(np.abs(want).max())
    err = float(np.abs(got[:n].double().numpy() - want).max())
    print(f"{what}: max|err| / peak = {err / peak:.2e}")
    assert err <= FP32_REL * peak, f"{what}: max |err| {err:.3e} > 1e-4 x peak {peak:.3e}"
    return err / peak


# ------------------------------------------------------------------------------------------------------ against float64
def test_the_reference_separates_plain_from_fast(items):
    """From the second iteration on, the plain and the textbook fast waveforms differ by more than 0.01 of the peak, a hundred
    times the bound below: no plain step passes for a fast one."""
    for T in FRAMES[1:]:
        it = items(T)
        for m in MOMENTA:
            for c in (2, 4):
                d = float(np.abs(it["fast"][m][c] - it["plain"][c]).max()) / float(np.abs(it["fast"][m][c]).max())
                assert d > 0.01, (T, m, c, d)


@pytest.mark.parametrize("T", FRAMES)
def test_against_float64_alone(gl, items, T):
    it = items(T)
    for m in MOMENTA:
        for n_iter in STEPS:
            got, alen = _iterate(gl, [it["M"]], [T], T + 1, n_iter, momentum=m)
            assert alen.tolist() == [256 * T]
            _check_item(got[0], it["fast"][m][n_iter], f"alone T={T}, momentum {m}, {n_iter} iterations")


@pytest.mark.parametrize("name", list(BATCHES))
def test_against_float64_ragged(gl, items, name):
    lens = BATCHES[name]
    Tp = max(lens) + 2
    for m in MOMENTA:
        for n_iter in STEPS:
            got, alen = _iterate(gl, [items(T)["M"] for T in lens], lens, Tp, n_iter, momentum=m)
            assert alen.tolist() == [256 * T for T in lens]
            for b, T in enumerate(lens):
                _check_item(got[b], items(T)["fast"][m][n_iter], f"batch {name} T={T}, momentum {m}, {n_iter} iterations")


def test_module_momentum_and_init(gl, items):
    """The module's own momentum is used without the argument, and `init` is x_0: iteration 1 the plain step of it."""
    it = items(17)
    got, _ = _iterate(gl, [it["M"]], [17], 18, 2)
    _check_item(got[0], it["fast"][0.99][2], "module momentum 0.99")
    half = FastGriffinLim(n_iter=2, momentum=0.5).to(DEV)
    got, _ = _iterate(half, [it["M"]], [17], 18, None)
    _check_item(got[0], it["fast"][0.5][2], "module momentum 0.5, module n_iter")
    start = it["x"] * 0.5
    start32 = torch.from_numpy(start).float().double().numpy()                  # the values the kernel reads
    for n_iter in (1, 2, 4):
        got, _ = _iterate(gl, [it["M"]], [17], 18, n_iter, init=[start])
        _check_item(got[0], fr.textbook(it["M"], n_iter, 0.99, init=start32), f"from init, {n_iter} iterations")


# --------------------------------------------------------------------------------------------- bit identity to the plain path
def test_bits_of_the_plain_path(gl, plain, items):
    lens = BATCHES["b"]
    Tp = max(lens) + 2
    mags = [items(T)["M"] for T in lens]
    for n_iter in (0, 1):                                                      # x_{-1} = 0: the first iteration is the plain step
        want, want_len = _iterate(plain, mags, lens, Tp, n_iter)
        got, got_len = _iterate(gl, mags, lens, Tp, n_iter)
        assert torch.equal(got, want) and torch.equal(got_len, want_len), f"n_iter={n_iter}"
    want, _ = _iterate(plain, mags, lens, Tp, 5)
    assert torch.equal(_iterate(gl, mags, lens, Tp, 5, momentum=0.0)[0], want)
    assert torch.equal(_iterate(FastGriffinLim(momentum=0).to(DEV), mags, lens, Tp, 5)[0], want)
    assert not torch.equal(_iterate(gl, mags, lens, Tp, 5)[0], want)
    xs = [items(T)["x"] * 0.5 for T in lens]                                   # from init: one step is the plain step of it
    assert torch.equal(_iterate(gl, mags, lens, Tp, 1, init=xs)[0], _iterate(plain, mags, lens, Tp, 1, init=xs)[0])


# --------------------------------------------------------------------------------------------------------------- full run
@pytest.mark.parametrize("kind,n", FULL_RUN)
def test_full_run_spectral_convergence(gl, plain, kind, n):
    T = n // 256
    x = synth.make_clip(kind, n, 0.5).double().numpy()
    M = np.abs(gr.stft(x)).astype(np.float32).astype(np.float64)
    ref = fr.textbook(M, 32, 0.99, seed=0, keep=COUNTS)
    waves = {c: _iterate(gl, [M], [T], T, c)[0][0].double().numpy() for c in COUNTS}          # each from scratch
    sc = [gr.spectral_convergence(waves[c], M) for c in COUNTS]
    sc_ref = [gr.spectral_convergence(ref[c], M) for c in COUNTS]
    rel = [abs(a - b) / b for a, b in zip(sc, sc_ref)]
    sc_plain = gr.spectral_convergence(_iterate(plain, [M], [T], T, 32)[0][0].double().numpy(), M)
    print(f"{kind}: spectral convergence {['%.5f' % v for v in sc]}, float64 {['%.5f' % v for v in sc_ref]}, relative "
          f"difference {['%.1e' % v for v in rel]}; plain after 32 {sc_plain:.5f}, ratio {sc[-1] / sc_plain:.3f}")
    assert max(rel) <= 1e-3, f"{kind}: spectral convergence {sc} against float64 {sc_ref}"
    assert sc[-1] <= 0.75 * sc_plain


# ----------------------------------------------------------------------------------------------------------- bit identity
def test_ragged_batch_equals_alone_and_ignores_padding(gl, items):
    lens = BATCHES["a"]
    Tp = max(lens) + 2
    mags = [items(T)["M"] for T in lens]
    base, base_len = _iterate(gl, mags, lens, Tp, 4)
    for b, T in enumerate(lens):                                           # an utterance alone, in a shorter row
        alone, _ = _iterate(gl, [mags[b]], [T], T + 1, 4)
        assert torch.equal(alone[0, :256 * T], base[b, :256 * T]), f"T={T}: the batch changed an utterance's bits"
    for fill in (0.0, 1e30):                                               # base ran with NaN past the lengths
        assert torch.equal(_iterate(gl, mags, lens, Tp, 4, fill=fill)[0], base), f"fill {fill}"
    assert torch.equal(_iterate(gl, mags, lens, Tp, 4)[0], base)           # a second call
    other, _ = _iterate(gl, mags, lens, Tp, 4, seed=1)                     # another seed: another start
    assert not torch.equal(other, base) and torch.equal(_iterate(gl, mags, lens, Tp, 4, seed=1)[0], other)
    # an init waveform with NaN / 0 / 1e30 past the lengths
    xs = [items(T)["x"] * 0.5 for T in lens]
    from_init, _ = _iterate(gl, mags, lens, Tp, 3, init=xs)
    for fill in (0.0, 1e30):
        assert torch.equal(_iterate(gl, mags, lens, Tp, 3, init=xs, fill=fill)[0], from_init), f"init fill {fill}"
    assert torch.isfinite(from_init).all() and not torch.equal(from_init, _iterate(gl, mags, lens, Tp, 3)[0])
    # device lengths outside [0, T]: zero rows, length 0
    wide = [np.concatenate([M, np.ones((Tp - M.shape[0], 513))]) for M in mags]      # finite everywhere
    bad, bad_len = _iterate(gl, wide, (-1, 2, Tp + 1, 33, 4), Tp, 4)
    assert bad_len.tolist() == [0, 512, 0, 256 * 33, 1024]
    assert (bad[0] == 0).all() and (bad[2] == 0).all()
    for b in (1, 3, 4):
        assert torch.equal(bad[b], base[b])


def test_every_count_lands_in_out_eagerly_and_replayed(gl, items):
    lens = BATCHES["a"]
    Tp = max(lens) + 2
    mag = _mag_batch([items(T)["M"] for T in lens], Tp)
    ln = torch.tensor(lens, dtype=torch.int64, device=DEV)
    for n_iter in (3, 4, 5):                                               # the three positions of the rotation
        want, want_len = _iterate(gl, [items(T)["M"] for T in lens], lens, Tp, n_iter)
        fresh, fresh_len = gl.from_magnitude(mag, ln, n_iter=n_iter)       # outputs of its own
        o = gl.empty_outputs(len(lens), Tp, DEV)
        g = graph.GraphedCall(lambda: gl.from_magnitude(mag, ln, n_iter=n_iter, out=o))
        o[0].zero_()
        o[1].zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(fresh.cpu(), want) and torch.equal(fresh_len.cpu(), want_len), f"n_iter={n_iter}"
        assert torch.equal(o[0].cpu(), want) and torch.equal(o[1].cpu(), want_len), f"n_iter={n_iter}, replayed"
    with pytest.raises(ValueError, match="nothing to iterate"):
        gl.from_magnitude(mag, ln, init=fresh, n_iter=0)
    e, el = gl.from_magnitude(mag[:, :0], None)
    assert e.shape == (len(lens), 0) and el.tolist() == [0] * len(lens)


# --------------------------------------------------------------------------------------- spectral convergence on the device
def _device_sc(gl, waves, mags, lens, Tp, fill=float("nan"), host=True):
    """waves float64 [n_b] each -> (the device's figures fp32 [B] on the CPU, the host's float64 figures of the same values;
    host=False: None, for magnitudes whose norm is 0)."""
    out = torch.full((len(waves) + 2,), SENTINEL, device=DEV)
    ln = torch.tensor(lens, dtype=torch.int64, device=DEV)
    got = gl.spectral_convergence(_audio_batch(waves, Tp, fill), _mag_batch(mags, Tp, fill), ln, out=out[:len(waves)])
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and (out[len(waves):] == SENTINEL).all()
    want = [gr.spectral_convergence(w, M) if len(w) else 0.0 for w, M in zip(waves, mags)] if host else None
    return got.cpu(), want


def _check_sc(got, want, what):
    worst = 0.0
    for b, (g, w) in enumerate(zip(got.tolist(), want)):
        if w == 0.0:
            assert g == 0.0, f"{what}[{b}]: {g} for an utterance without frames"
        elif w >= 0.01:
            print(f"{what}[{b}]: device {g:.7f}, float64 {w:.7f}, relative difference {abs(g - w) / w:.1e}")
            assert abs(g - w) <= 1e-5 * w, f"{what}[{b}]: device {g} against float64 {w}"
            worst = max(worst, abs(g - w) / w)
    return worst


@pytest.fixture(scope="module")
def iterates(gl, items):
    """(T, count) -> the GPU's waveform after `count` fast iterations (float64 holding fp32 values), made once."""
    cache = {}

    def get(T, count):
        if (T, count) not in cache:
            cache[T, count] = _iterate(gl, [items(T)["M"]], [T], T + 1, count)[0][0, :256 * T].double().numpy()
        return cache[T, count]
    return get


@pytest.mark.parametrize("T", FRAMES)
def test_device_spectral_convergence_alone(gl, items, iterates, T):
    for count in (0, 1, 8):
        got, want = _device_sc(gl, [iterates(T, count)], [items(T)["M"]], [T], T + 1)
        assert T == 0 or want[0] >= 0.01
        _check_sc(got, want, f"alone T={T} after {count}")


@pytest.mark.parametrize("name", list(BATCHES))
def test_device_spectral_convergence_ragged(gl, items, iterates, name):
    lens = BATCHES[name]
    Tp = max(lens) + 2
    mags = [items(T)["M"] for T in lens]
    for count in (0, 1, 8):
        waves = [iterates(T, count) for T in lens]
        got, want = _device_sc(gl, waves, mags, lens, Tp)
        _check_sc(got, want, f"batch {name} after {count}")
        for b, T in enumerate(lens):                                       # ragged = alone, bit for bit
            alone, _ = _device_sc(gl, [waves[b]], [mags[b]], [T], T + 1)
            assert torch.equal(alone[0], got[b]), f"T={T}: the batch changed an utterance's figure"
        for fill in (0.0, 1e30):                                           # NaN past the lengths above
            assert torch.equal(_device_sc(gl, waves, mags, lens, Tp, fill=fill)[0], got), f"fill {fill}"


def test_device_spectral_convergence_edge_cases(gl, plain, items):
    lens = BATCHES["b"]
    Tp = max(lens) + 1
    xs, mags = [items(T)["x"] for T in lens], [items(T)["M"] for T in lens]
    own, _ = _device_sc(plain, xs, mags, lens, Tp)                          # a clip with its own magnitude; the base class has it
    print(f"own magnitude: {own.tolist()}")
    assert float(own.max()) <= 1e-5 and float(own.min()) >= 0.0
    zeros = [np.zeros((T, 513)) for T in lens]
    silent, _ = _device_sc(gl, [np.zeros(256 * T) for T in lens], zeros, lens, Tp, host=False)
    assert (silent == 0).all()
    loud, _ = _device_sc(gl, xs, zeros, lens, Tp, host=False)
    assert torch.isinf(loud).all() and (loud > 0).all()
    # lengths out of range count as 0; the others keep their bits
    wide = [np.concatenate([M, np.ones((Tp - M.shape[0], 513))]) for M in mags]
    long = [np.concatenate([x, np.zeros(256 * Tp - len(x))]) for x in xs]
    base, _ = _device_sc(gl, xs, mags, lens, Tp)
    ln = torch.tensor((-1, 3, Tp + 1, 17, 32), dtype=torch.int64, device=DEV)
    bad = gl.spectral_convergence(_audio_batch(long, Tp), _mag_batch(wide, Tp), ln).cpu()
    assert bad[0] == 0 and bad[2] == 0 and torch.equal(bad[[1, 3, 4]], base[[1, 3, 4]])
    # without lengths every frame counts; zero frames give 0
    full, want = _device_sc(gl, [xs[4] * 0.5], [mags[4]], [32], 32)
    none = gl.spectral_convergence(_audio_batch([xs[4] * 0.5], 32), _mag_batch([mags[4]], 32)).cpu()
    assert torch.equal(none, full) and abs(float(full[0]) - want[0]) <= 1e-5 * want[0] and want[0] > 0.4
    empty = gl.spectral_convergence(torch.empty((3, 0), device=DEV), torch.empty((3, 0, 513), device=DEV),
                                    out=torch.full((3,), SENTINEL, device=DEV))
    assert empty.tolist() == [0.0] * 3


def test_device_spectral_convergence_in_a_graph(gl, items):
    lens = BATCHES["a"]
    Tp = max(lens) + 2
    mag = _mag_batch([items(T)["M"] for T in lens], Tp)
    ln = torch.tensor(lens, dtype=torch.int64, device=DEV)
    wav, sc = gl.empty_outputs(len(lens), Tp, DEV), torch.empty(len(lens), device=DEV)

    def call():
        audio, _ = gl.from_magnitude(mag, ln, n_iter=4, out=wav)
        return gl.spectral_convergence(audio, mag, ln, out=sc)

    eager = call().clone()
    g = graph.GraphedCall(call)
    sc.fill_(SENTINEL)
    wav[0].zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(sc, eager) and eager[0] == 0 and (eager[1:] > 0.01).all() and (eager[1:] < 1).all()


# ----------------------------------------------------------------------------------------------------------- whole chain
def test_text_to_pcm16_as_one_graph():
    """text -> mel -> FastGriffinLim -> conditioned -> PCM16, captured as one HIP graph: the replay equals the eager chain
    (tests/test_gpu_griffinlim.py's chain and inputs, with the fast iteration)."""
    from isp_tts_amd.data import AudioConditioner, to_pcm16
    model = _acoustic_model()
    gl = FastGriffinLim(n_iter=4).to(DEV)
    cond = AudioConditioner(22050)
    inp = synth.make_inputs(3, 30, 64, variable=True, seed=21)
    text, tl, x_t = inp["text"].to(DEV), inp["text_len"].to(DEV), inp["flow_x0"].to(DEV)
    dur = torch.full((3, 30), 2, dtype=torch.int64, device=DEV)
    wav = gl.empty_outputs(3, 64, DEV)
    out = cond.empty_outputs(3, wav[0].shape[1], DEV)
    pcm = torch.empty(wav[0].shape, dtype=torch.int16, device=DEV)

    def chain():
        mel, ao = model.infer(text, text_lengths=tl, duration_target=dur, steps=4, flow_noise=x_t, max_dec_len=64)
        audio, audio_len = gl(mel, ao.dec_lengths, out=wav)
        r = cond(audio, audio_len, out=out)
        return to_pcm16(r["audio"], r["audio_len"], out=pcm), r, mel, ao.dec_lengths

    _, _, mel, dec = chain()
    torch.cuda.synchronize()
    eager_pcm, eager_wav, eager = pcm.clone(), wav[0].clone(), {k: v.clone() for k, v in out.items()}
    assert (wav[1] >= 256).all() and float(wav[0].abs().max()) > 0
    assert not torch.equal(GriffinLim(n_iter=4).to(DEV)(mel, dec)[0], eager_wav)           # the momentum acts in the chain
    g = graph.GraphedCall(lambda: chain()[:2])
    pcm.zero_()
    wav[0].zero_()
    for v in out.values():
        v.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(pcm, eager_pcm) and torch.equal(wav[0], eager_wav)
    for k in eager:
        assert eager[k].cpu().numpy().tobytes() == out[k].cpu().numpy().tobytes(), k
    assert (out["audio_len"] > 0).all() and pcm.abs().max() > 100


def test_no_aten_compute_ops(gl, items):
    from torch.utils._python_dispatch import TorchDispatchMode
    harmless = ("aten.view", "aten.empty", "aten._unsafe_view", "aten.transpose", "aten.slice", "aten.select",
                "aten.unsqueeze", "aten.expand", "aten.detach", "aten.alias", "aten.t.", "aten.permute", "aten.squeeze",
                "aten.reshape", "aten.as_strided", "aten.is_", "aten.size", "aten.stride", "aten.lift_fresh",
                "aten._reshape_alias", "aten.split", "aten.unbind", "aten.sym_", "aten.empty_like", "aten.new_empty",
                "aten.record_stream")
    seen = []

    class Watch(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            if not str(func).startswith(harmless):
                seen.append(str(func))
            return func(*args, **(kwargs or {}))

    mel = torch.full((2, 80, 18), -3.0, device=DEV)
    ln = torch.tensor([17, 4], dtype=torch.int64, device=DEV)
    out, init = gl.empty_outputs(2, 18, DEV), torch.zeros((2, 256 * 18), device=DEV)
    sc = torch.empty(2, device=DEV)
    gl(mel, ln)
    torch.cuda.synchronize()
    with Watch():
        gl(mel, ln)
        audio, _ = gl(mel, ln, out=out)
        gl(mel, None)
        mag = gl.magnitude(mel, ln)
        gl.from_magnitude(mag, ln, n_iter=0)
        gl.from_magnitude(mag, ln, init=init, n_iter=5, seed=5, out=out, momentum=0.5)
        gl.spectral_convergence(audio, mag, ln)
        gl.spectral_convergence(audio, mag, None, out=sc)
        gl.spectral_convergence(audio[:, :0], mag[:, :0], ln)
    torch.cuda.synchronize()
    assert not seen, f"PyTorch compute ops inside FastGriffinLim: {sorted(set(seen))}"
