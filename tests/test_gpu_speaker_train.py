"""GPU: multi-speaker training (`AcousticModel(speaker_in_forward=True)`).

The two kernels - ispk_add_speaker_out_f32, ispk_speaker_grad_f32 - against float64 at the smallest shapes where they can go
wrong, and the model - teacher-forced forward, the training step in both duration modes, fp32 and bf16 AMP, the captured step, a
new-voice fine-tune, the evaluator - against outputs of the reference itself with `speaker_encoder` read as `speaker_embedding`
(tests/golden/speaker_train.npz, tools/make_speaker_train_goldens.py)."""
import numpy as np
import pytest
import torch

from conftest import crc, golden

import hard_duration_reference as hdr
from amp_bounds import AMP_GRAD_NORM_RTOL, AMP_GRAD_SAMPLE, AMP_LOSS_RTOL, AMP_SLOPE_FAMILY, tensor_class
from isp_tts_amd import graph, runtime, synth, train
from isp_tts_amd.acoustic import AcousticModel, AcousticModelEvaluator
from isp_tts_amd.config import AcousticDims

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24                  # unit roundoff of fp32
BATCH_KEYS = ("text", "text_len", "mel", "mel_len", "pitch", "energy")


def _maxdiff(a, b) -> float:
    a = a.detach().cpu() if isinstance(a, torch.Tensor) else torch.as_tensor(a)
    return float((a.double() - torch.as_tensor(b).double()).abs().max())


# ------------------------------------------------------------------------------------------------------------ the kernels
_IDS_1 = [[2], [5], [2], [0], [2]]
_LEN_1 = [37, 1, 20, 36, 9]
GRAD_CASES = {   # name -> (B, L, D, S, ids, text_len): L = 37 is two full 16-row chunks and one of 5; 20 ends inside a chunk
    "repeated_and_absent": (5, 37, 384, 7, _IDS_1, _LEN_1),
    "one_id_no_lengths": (3, 8, 132, 4, [1], None),                 # a single id (stride 0), D no multiple of 256, every row counts
    "big_table": (2, 5, 384, 1307, [[1306], [0]], [5, 2]),
    "clamped_ids": (5, 37, 384, 7, [[2], [-3], [2], [9], [2]], _LEN_1),   # -3 -> 0 and 9 -> 6, as the forward kernel clamps
}


def _grad_case(name):
    B, L, D, S, ids, text_len = GRAD_CASES[name]
    g = torch.Generator().manual_seed(11)
    d_x = torch.randn(B, L, D, generator=g)
    ids = torch.tensor(ids, dtype=torch.int64)
    tl = torch.tensor(text_len) if text_len is not None else None
    counted = torch.ones(B, L, dtype=torch.bool) if tl is None else torch.arange(L)[None] < tl[:, None]
    row = ids.view(-1).clamp(0, S - 1).expand(B)
    x64 = d_x.double() * counted[..., None]
    want = torch.zeros(S, D, dtype=torch.float64).index_add_(0, row, x64.sum(dim=1))
    mag = torch.zeros(S, D, dtype=torch.float64).index_add_(0, row, x64.abs().sum(dim=1))        # sum of |addends|
    n = torch.zeros(S, dtype=torch.float64).index_add_(0, row, counted.sum(dim=1).double())      # number of addends
    d_x = d_x.masked_fill(~counted[..., None], float("nan"))        # rows at l >= text_len[b] must never be read
    return d_x, ids, tl, S, want, mag, n


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("case", list(GRAD_CASES))
def test_speaker_grad_against_float64(case, accumulate):
    """ispk_speaker_grad_f32 against a float64 `index_add` over the counted rows.  Allowed error per value: n 2^-24 sum|addends|
    for n addends, the bound of an fp32 sum in ANY order (with `accumulate` the prior content is one more addend).  NaNs sit in
    every row the kernel must leave out."""
    d_x, ids, tl, S, want, mag, n = _grad_case(case)
    prior = torch.randn(want.shape, generator=torch.Generator().manual_seed(3)) if accumulate else None
    out = prior.to(DEV) if accumulate else None
    got = runtime.speaker_grad(d_x.to(DEV), ids.to(DEV), S, tl.to(DEV) if tl is not None else None, out=out, accumulate=accumulate)
    torch.cuda.synchronize()
    got = got.cpu()
    assert not torch.isnan(got).any()
    if accumulate:
        want, mag, n = want + prior.double(), mag + prior.abs().double(), n + 1
    err = (got.double() - want).abs()
    bound = n[:, None] * U * mag
    print(f"{case} accumulate={accumulate}: worst error / bound = {float((err / bound.clamp(min=1e-300)).max()):.3f}, "
          f"up to {int(n.max())} addends")
    assert bool((err <= bound).all())
    absent = n == (1 if accumulate else 0)
    assert bool(absent.any()) and torch.equal(got[absent], prior[absent] if accumulate else torch.zeros_like(got[absent]))
    if case == "big_table":
        assert int(absent.sum()) == 1305 and not absent[0] and not absent[1306]
    if case == "clamped_ids":
        assert not absent[0] and not absent[6] and bool(absent[5])


def test_speaker_grad_gives_the_same_bits_twice():
    d_x, ids, tl, S, *_ = _grad_case("repeated_and_absent")
    args = (d_x.to(DEV), ids.to(DEV), S, tl.to(DEV))
    first = runtime.speaker_grad(*args)
    again = runtime.speaker_grad(*args)
    torch.cuda.synchronize()
    assert torch.equal(first, again) and bool(first.any())


def test_speaker_grad_refuses_what_it_was_not_built_for():
    lib = runtime.lib()
    x = torch.zeros(1, 513, 8, device=DEV)
    ids = torch.zeros(1, 1, dtype=torch.int64, device=DEV)
    table = torch.zeros(2, 8, device=DEV)
    ws = torch.zeros(64 * 1024, device=DEV)
    call = lambda L, D, floats: lib.ispk_speaker_grad_f32(x.data_ptr(), ids.data_ptr(), 1, None, ws.data_ptr(), floats,   # noqa: E731
                                                          table.data_ptr(), 8, 2, 1, L, D, 0, None)
    assert call(513, 8, ws.numel()) == -2                           # L > 512
    assert call(64, 6, ws.numel()) == -3                            # D no multiple of 4
    assert call(64, 8, 4 * 8 - 1) == -2                             # workspace one float short of B * ceil(L / 16) * D
    assert call(64, 8, 4 * 8) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", ["repeated_and_absent", "one_id_no_lengths", "clamped_ids"])
def test_add_speaker_out_of_place_equals_the_in_place_kernel(case):
    B, L, D, S, ids, _ = GRAD_CASES[case]
    g = torch.Generator().manual_seed(5)
    x, table = torch.randn(B, L, D, generator=g).to(DEV), torch.randn(S, D, generator=g).to(DEV)
    ids = torch.tensor(ids, dtype=torch.int64, device=DEV)
    before = x.clone()
    out = runtime.add_speaker(x, table, ids)
    want = runtime.add_speaker_(x.clone(), table, ids)
    torch.cuda.synchronize()
    assert torch.equal(x, before) and out.data_ptr() != x.data_ptr()
    assert torch.equal(out, want) and not torch.equal(out, x)
    row = ids.view(-1).clamp(0, S - 1).expand(B)
    assert torch.equal(out, x + table[row][:, None, :])
    with pytest.raises(ValueError, match="does not broadcast"):
        runtime.add_speaker(x, table, torch.zeros(B + 1, 1, dtype=torch.int64, device=DEV))


# ------------------------------------------------------------------------------------------------------------ the model
SPEAKERS = 4


def _model(state_dict, soft=True):
    """The 4-speaker model with the switch on and the fixture's weights, in eval mode (no dropout draws), trainable."""
    runtime.lib()
    model = AcousticModel.init(dict(AcousticDims().model_config(soft_duration=soft), num_speakers=SPEAKERS), speaker_in_forward=True)
    sd = dict(state_dict)
    sd["speaker_embedding.weight"] = synth.make_speaker_table(SPEAKERS)
    model.load_state_dict(sd, strict=True)
    return model.to(DEV).eval()


@pytest.fixture(scope="module")
def fixture_and_inputs():
    g = golden("speaker_train.npz")
    inp = hdr.fixture_inputs()
    assert [crc(inp[k]) for k in ("text", "mel", "pitch", "energy")] == [int(v) for v in g["inputs_crc"]]
    inp["speaker"] = torch.from_numpy(g["speaker"])
    return g, {k: v.to(DEV) for k, v in inp.items()}


@pytest.fixture(scope="module")
def frozen_model(state_dict):
    return _model(state_dict).requires_grad_(False)


@pytest.fixture(scope="module")
def forward_out(frozen_model, fixture_and_inputs):
    _, inp = fixture_and_inputs
    with torch.no_grad():
        out = frozen_model(**inp)
    torch.cuda.synchronize()
    return out


def test_forward_against_the_reference_fixture(frozen_model, forward_out, fixture_and_inputs):
    """The tape-free forward, fp32, with the bounds of test_gpu_hard_duration.py::test_forward_against_the_reference_fixture;
    other ids move the mel of the utterance they belong to."""
    g, inp = fixture_and_inputs
    ao = forward_out.adaptor_output
    d = {"mel": _maxdiff(forward_out.mel[:, :, ::int(g["mel_row_step"])], g["mel_rows"]),
         "log_duration": _maxdiff(ao.log_duration, g["log_duration"]),
         "flow_loss": abs(float(ao.losses["flow_loss"]) - float(g["flow_loss"]))}
    print("multi-speaker forward vs reference: " + ", ".join(f"{k} {v:.2e}" for k, v in d.items()))
    assert np.array_equal(ao.dec_lengths.cpu().numpy(), g["dec_lengths"])
    assert forward_out.mel.shape == (2, 80, 512) and d["mel"] <= 1e-4
    assert d["log_duration"] < 1e-4 and d["flow_loss"] < 1e-5
    with torch.no_grad():
        other = frozen_model(**dict(inp, speaker=torch.tensor([[3], [3]], device=DEV)))
    moved = _maxdiff(other.mel[1], forward_out.mel[1].cpu())
    print(f"ids [[3],[3]] move the mel of item 1 by {moved:.3f} (the reference: {float(g['mel_moved']):.3f})")
    assert moved > 0.1
    with pytest.raises(ValueError, match="speaker"):
        frozen_model(**{k: v for k, v in inp.items() if k != "speaker"})


def test_evaluator_runs_on_the_tape_free_forward(forward_out, fixture_and_inputs):
    """The trainer's evaluation loop: `AcousticModelEvaluator` on what the `no_grad` forward of the switched-on model returns."""
    _, inp = fixture_and_inputs
    metrics = AcousticModelEvaluator()(inp, forward_out)
    torch.cuda.synchronize()
    assert len(metrics) == 3 and all(bool(torch.isfinite(v)) for v in metrics.values()), metrics


def test_graphed_forward_takes_the_ids_as_a_static_input(frozen_model, forward_out, fixture_and_inputs):
    _, inp = fixture_and_inputs
    gf = graph.GraphedForward(frozen_model, *(inp[k] for k in BATCH_KEYS), flow_noise=inp["flow_noise"], flow_time=inp["flow_time"],
                              speaker=inp["speaker"])
    assert torch.equal(gf.replay().mel, forward_out.mel)
    ids = torch.tensor([[0], [2]], device=DEV)
    mel = gf(speaker=ids).mel.clone()
    with torch.no_grad():
        eager = frozen_model(**dict(inp, speaker=ids))
    torch.cuda.synchronize()
    assert torch.equal(mel, eager.mel) and not torch.equal(mel, forward_out.mel)
    with pytest.raises(NotImplementedError, match="speaker"):
        graph.SegmentedForward(frozen_model, *(inp[k] for k in BATCH_KEYS))


def test_batch_ingest_stages_the_ids_with_the_batch(frozen_model, fixture_and_inputs, forward_out):
    """`ingest.BatchIngest` on the GPU: a collator-layout host batch with a `speaker` field comes back as device tensors whose
    `model_inputs` drive the forward to the same mel; a batch without the field comes back without it."""
    from isp_tts_amd import ingest
    _, inp = fixture_and_inputs
    host = {"text_vector": inp["text"].cpu(), "text_vector_len": inp["text_len"].cpu(), "mel": inp["mel"].cpu(),
            "mel_len": inp["mel_len"].cpu(), "pitch": inp["pitch"].cpu(), "energy": inp["energy"].cpu(), "speaker": inp["speaker"].cpu()}
    ing = ingest.BatchIngest(DEV, max_batch=4, max_text=100, max_mel=512, slots=2)
    ing.submit(host)
    ing.submit({k: v for k, v in host.items() if k != "speaker"})
    kw = ingest.model_inputs(ing.get())
    assert kw["speaker"].is_cuda and kw["speaker"].dtype == torch.int64 and torch.equal(kw["speaker"], inp["speaker"])
    with torch.no_grad():
        out = frozen_model(**kw, flow_noise=inp["flow_noise"], flow_time=inp["flow_time"])
    ing.done()
    assert "speaker" not in ingest.model_inputs(ing.get())
    ing.done()
    torch.cuda.synchronize()
    assert torch.equal(out.mel, forward_out.mel)


def _step(model, inp, amp):
    return train.acoustic_train_forward(model, *(inp[k] for k in BATCH_KEYS), flow_noise=inp["flow_noise"], flow_time=inp["flow_time"],
                                        amp=amp, train_aligner=True, speaker=inp["speaker"])


def _sample(t, n=192):
    f = t.detach().reshape(-1)
    return f[::max(1, -(-f.numel() // n))].cpu()


def _check_absent_rows(table_grad, g):
    assert not table_grad[[int(s) for s in g["absent"]]].any(), "a speaker absent from the batch has a gradient"


@pytest.mark.parametrize("mode", ["soft", "hard"])
def test_training_step_against_the_reference_fixture(state_dict, fixture_and_inputs, mode):
    """fp32, with the tolerances of test_gpu_hard_duration.py::test_training_step_against_the_reference_fixture: the four losses
    and the total to 2e-4, every one of the 207 gradients - norm and (soft: the fixture's hard half keeps norms only) strided
    sample - to 2e-3 of the tensor's scale; the table's gradient whole to 2e-3 of its largest entry, rows 0 and 2 exactly zero."""
    g, inp = fixture_and_inputs
    model = _model(state_dict, soft=mode == "soft")
    names = [str(n) for n in g["names"]]
    params = dict(model.named_parameters())
    assert list(params) == names and len(names) == 207
    _, total, losses = _step(model, inp, amp=False)
    for k, v in losses.items():
        ref = float(g[f"{mode}_loss_" + k.replace("/", "_")])
        assert abs(v.item() - ref) < 2e-4 * max(abs(ref), 1.0), (k, v.item(), ref)
    assert abs(total.item() - float(g[f"{mode}_loss_total"])) < 2e-4 * float(g[f"{mode}_loss_total"])
    total.backward()
    worst = 0.0
    for i, n in enumerate(names):
        gr, scale, ref_norm = params[n].grad, float(g[f"{mode}_grad_absmax"][i]), float(g[f"{mode}_grad_norm"][i])
        assert gr is not None, n
        assert abs(gr.double().norm().item() - ref_norm) <= 2e-3 * ref_norm + 1e-7, n
        if mode == "soft":
            err = (_sample(gr) - torch.from_numpy(g[f"soft_g{i}"])).abs().max().item() / max(scale, 1e-12)
            worst = max(worst, err)
            assert err <= 2e-3, (n, err)
    table, ref = model.speaker_embedding.weight.grad.cpu(), torch.from_numpy(g[f"{mode}_table_grad"])
    e_table = _maxdiff(table, ref) / float(ref.abs().max())
    print(f"{mode}: worst sampled gradient error {worst:.2e} of the tensor's scale; table gradient {e_table:.2e} of its largest entry")
    assert e_table <= 2e-3
    _check_absent_rows(table, g)


@pytest.mark.parametrize("mode", ["soft", "hard"])
def test_amp_training_step_against_the_reference_fixture(state_dict, fixture_and_inputs, mode):
    """The same step under bf16 AMP within the stated bounds of tests/amp_bounds.py, in the form of test_gpu_train_loop.py's test
    against train.npz: losses to AMP_LOSS_RTOL, per tensor the norm to AMP_GRAD_NORM_RTOL and the sampled entries to AMP_GRAD_SAMPLE
    (ALiBi slopes: that file's family bound over the whole 6-element tensor); the table counts as "general" and is compared whole.
    The fixture's hard half keeps norms only: there the slopes, whose own norm is no scale for their error, are not compared."""
    g, inp = fixture_and_inputs
    model = _model(state_dict, soft=mode == "soft")
    names = [str(n) for n in g["names"]]
    params = dict(model.named_parameters())
    _, total, losses = _step(model, inp, amp=True)
    for k, v in list(losses.items()) + [("total", total)]:
        ref = float(g[f"{mode}_loss_" + k.replace("/", "_")])
        assert abs(v.item() - ref) <= AMP_LOSS_RTOL * max(abs(ref), 1e-3), (k, v.item(), ref)
    total.backward()
    slope_scale = max(float(g[f"{mode}_grad_norm"][i]) for i, n in enumerate(names) if tensor_class(n) == "slope")
    worst_n, worst_s = (0.0, ""), (0.0, "")
    for i, n in enumerate(names):
        gr, scale, ref_norm = params[n].grad, float(g[f"{mode}_grad_absmax"][i]), float(g[f"{mode}_grad_norm"][i])
        assert gr is not None, n
        if tensor_class(n) == "slope":
            if mode == "soft":
                ref_s = torch.from_numpy(g[f"soft_g{i}"])
                assert ref_s.numel() == gr.numel()
                assert float((gr.detach().reshape(-1).cpu().double() - ref_s.double()).norm()) / slope_scale <= AMP_SLOPE_FAMILY, n
            continue
        e_n = abs(gr.double().norm().item() - ref_norm) / max(ref_norm, 1e-12)
        worst_n = max(worst_n, (e_n, n))
        assert e_n <= AMP_GRAD_NORM_RTOL, (n, e_n)
        if mode == "soft":
            e_s = (_sample(gr) - torch.from_numpy(g[f"soft_g{i}"])).abs().max().item() / max(scale, 1e-12)
            worst_s = max(worst_s, (e_s, n))
            assert e_s <= AMP_GRAD_SAMPLE, (n, e_s)
    assert tensor_class("speaker_embedding.weight") == "general"
    table, ref = model.speaker_embedding.weight.grad.cpu(), torch.from_numpy(g[f"{mode}_table_grad"])
    e_table = _maxdiff(table, ref) / float(ref.abs().max())
    print(f"{mode} AMP: worst norm error {worst_n[0]:.2e} ({worst_n[1]}), worst sampled entry {worst_s[0]:.2e} ({worst_s[1]}), "
          f"table gradient {e_table:.2e} of its largest entry")
    assert e_table <= AMP_GRAD_SAMPLE
    _check_absent_rows(table, g)


# ------------------------------------------------------------------------------------------------------------ the captured step
def _small_batch():
    d = {k: v.to(DEV) for k, v in synth.make_inputs(3, 52, 160, variable=True, seed=9).items()}
    return {k: d[k] for k in BATCH_KEYS + ("flow_x0", "flow_t")}


def test_graphed_training_step_replays_match_eager_steps(state_dict):
    """`train.GraphedTrainStep` with a `speaker` field, in the form of test_gpu_hard_duration.py's test of this name: two warm-up
    steps on the capture batch, then three replays with OTHER ids each give bit for bit the parameters of the same five eager
    steps - the replay reads the ids it was handed, not the ones it was captured with."""
    def make():
        torch.manual_seed(11)
        m = _model(state_dict)
        o = train.FlatAdamW(list(m.parameters()), lr=2e-4, weight_decay=1e-2, grad_clip=1.0)
        o.check_finite = False
        return m, o
    batch = _small_batch()
    ids = [torch.tensor(v, device=DEV) for v in ([[0], [1], [2]], [[3], [3], [0]], [[1], [0], [3]], [[2], [2], [2]])]
    m_e, o_e = make()
    eager_tot = []
    for step_ids in [ids[0], ids[0]] + ids[1:]:
        _, total, _ = train.acoustic_train_forward(m_e, *(batch[k] for k in BATCH_KEYS), flow_noise=batch["flow_x0"],
                                                   flow_time=batch["flow_t"], amp=True, speaker=step_ids)
        o_e.step(total)
        eager_tot.append(float(total.detach()))
    m_g, o_g = make()
    step = train.GraphedTrainStep(m_g, o_g, dict(batch, speaker=ids[0]), amp=True, warmup=2)
    graph_tot = [float(step(**dict(batch, speaker=step_ids))[0].detach()) for step_ids in ids[1:]]
    torch.cuda.synchronize()
    assert o_g.step_count == 5 and o_e.step_count == 5
    assert graph_tot == eager_tot[2:], f"losses: graph {graph_tot} vs eager {eager_tot[2:]}"
    assert torch.equal(o_g.flat.data, o_e.flat.data) and torch.equal(o_g.exp_avg_sq, o_e.exp_avg_sq)
    assert torch.equal(m_g.speaker_embedding.weight, m_e.speaker_embedding.weight)
    step.close()


def test_graphed_training_step_reads_the_ids_of_each_replay(state_dict):
    """Two replays with different ids give different losses, two with the same ids the same one: with lr = 0 and no weight decay
    the parameters stand still (and eval mode draws no dropout), so nothing but the ids differs between the replays."""
    model = _model(state_dict)
    opt = train.FlatAdamW(list(model.parameters()), lr=0.0, weight_decay=0.0, grad_clip=1.0)
    opt.check_finite = False
    batch = _small_batch()
    a, b = torch.tensor([[0], [1], [2]], device=DEV), torch.tensor([[0], [3], [2]], device=DEV)
    evaluator = AcousticModelEvaluator()
    step = train.GraphedTrainStep(model, opt, dict(batch, speaker=a), amp=True, warmup=1, evaluator=evaluator)
    tot = [float(step(speaker=s)[0].detach()) for s in (a, b, a)]
    metrics = {k: float(v) for k, v in step.metrics.items()}
    torch.cuda.synchronize()
    assert tot[0] == tot[2] and tot[0] != tot[1], tot
    assert all(np.isfinite(v) for v in metrics.values()), metrics
    step.close()


def test_new_voice_fine_tune_moves_only_the_table(state_dict, fixture_and_inputs):
    """`extend_speakers(1)`, `freeze(["speaker_embedding"])`, then a FlatAdamW (lr 2e-4, weight decay 1e-2): one step on a batch of
    the new id alone leaves every other parameter bit-identical, moves the new row, and applies to the old rows - zero gradient,
    zero moments - the decoupled decay alone: row (1 - lr weight_decay), to 1 ulp."""
    _, inp = fixture_and_inputs
    lr, wd = 2e-4, 1e-2
    model = _model(state_dict)
    new = model.extend_speakers(1)
    assert new == SPEAKERS and model.speaker_embedding.weight.is_cuda
    model.freeze(["speaker_embedding"])
    opt = train.FlatAdamW(model.parameters(), lr=lr, weight_decay=wd)
    assert [tuple(p.shape) for p in opt.flat.params] == [(SPEAKERS + 1, 384)]
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    ids = torch.full((2, 1), new, dtype=torch.int64, device=DEV)
    _, total, _ = train.acoustic_train_forward(model, *(inp[k] for k in BATCH_KEYS), flow_noise=inp["flow_noise"],
                                               flow_time=inp["flow_time"], amp=False, train_aligner=False, speaker=ids)
    opt.step(total)
    torch.cuda.synchronize()
    for n, p in model.named_parameters():
        if n != "speaker_embedding.weight":
            assert torch.equal(p, before[n]), n
    table, old = model.speaker_embedding.weight.detach().cpu(), before["speaker_embedding.weight"].cpu()
    assert not torch.equal(table[new], old[new])
    moved = float((table[new] - old[new]).abs().max())
    want = old[:new].double() * (1.0 - lr * wd)
    ulp = torch.from_numpy(np.spacing(want.float().abs().numpy())).double()
    off = (table[:new].double() - want).abs() / ulp
    print(f"new-voice step: the new row moved by up to {moved:.2e}; old rows within {float(off.max()):.2f} ulp of row (1 - lr wd)")
    assert bool((off <= 1.0).all()) and not torch.equal(table[:new], old[:new])
