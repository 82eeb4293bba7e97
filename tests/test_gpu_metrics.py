"""GPU: the evaluator (models/acoustic/evaluator.py) - ispk_acoustic_metrics_f32 against a float64 restatement computed on the
GPU from the same operands, across batch sizes, frame counts on and around the 32-frame chunk edges, text widths, ragged lengths,
argmax ties and operand layouts; against the REAL reference's values (tests/golden/metrics.npz); and end to end behind the
reference's loop body, with and without a tape, eagerly and inside the captured training step."""
import math
import zlib

import numpy as np
import pytest
import torch

from conftest import crc, golden

from isp_tts_amd import runtime, synth, train
from isp_tts_amd.acoustic import MCD, AcousticModelEvaluator, AlignmentMetric, create_dct

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS32 = 2.0 ** -24
LOGDB = 10.0 * math.sqrt(2.0) / math.log(10.0)


# ---------------------------------------------------------------------------------------------------- float64 restatement
def _frames(x, C):
    """[B, T, C] float64 as MCD._mfcc reads a mel (evaluator.py:28-31)."""
    return (x if x.shape[-1] == C else x.transpose(1, 2)).double()


def first_argmax(a):
    """Index of the first maximum of each row (independent of torch.argmax)."""
    mx = a.max(dim=-1, keepdim=True).values
    idx = torch.arange(a.shape[-1], device=a.device).expand_as(a)
    return torch.where(a == mx, idx, a.shape[-1]).min(dim=-1).values


def ref64(mel_out, mel_target, mel_len, text_len, attn, dct):
    C = dct.shape[0]
    ml, tl = mel_len.double(), text_len.double()
    d = _frames(mel_out, C) - _frames(mel_target, C)
    cep = (d @ dct.double())[..., 1:]
    mcd = LOGDB * ((cep * cep).sum(-1).sqrt().sum(-1) / ml).mean()
    a = first_argmax(attn.double())
    T = attn.shape[1]
    steps = (1.0 + (a[:, 1:] - a[:, :-1]).double() ** 2).sqrt()
    valid = torch.arange(1, T, device=attn.device)[None, :] < mel_len[:, None]
    length = ((steps * valid).sum(-1) / (tl * tl + ml * ml).sqrt()).mean()
    strength = attn.double().max(dim=-1).values.sum() / ml.sum()
    return torch.stack([mcd, length, strength])


# ---------------------------------------------------------------------------------------------------- operands
def _mel_pair(g, B, C, T, layout, mel_len):
    """(mel_out, mel_target) views in `layout`: "bct" [B, C, T], "btc" [B, T, C], "quirk" [B, 80, 80] read frames-first,
    "pad_bct" / "pad_btc" the same as views into NaN-filled buffers with padded batch / channel / frame strides,
    "mixed" out [B, C, T] with target [B, T, C]."""
    tgt = torch.randn(B, T, C, generator=g) * 2.0 - 5.0
    tgt = tgt * (torch.arange(T)[None, :, None] < mel_len[:, None, None].cpu())
    out = tgt + 0.5 * torch.randn(B, T, C, generator=g)
    views = []
    for k, x in enumerate((out, tgt)):
        x = x.to(DEV)
        if layout in ("btc", "quirk") or (layout == "mixed" and k == 1):
            views.append(x.contiguous())
        elif layout in ("bct", "mixed"):
            views.append(x.transpose(1, 2).contiguous())
        elif layout == "pad_bct":     # channel stride T + 7, batch stride (C + 2)(T + 7): element loads
            buf = torch.full((B + 1, C + 2, T + 7), float("nan"), device=DEV)
            v = buf[1:, 1:C + 1, 3:T + 3]
            v.copy_(x.transpose(1, 2))
            views.append(v)
        elif layout == "pad_btc":     # frame stride C + 4: float4 loads along the channels
            buf = torch.full((B + 2, T + 3, C + 4), float("nan"), device=DEV)
            v = buf[1:B + 1, 2:T + 2, 4:C + 4]
            v.copy_(x)
            views.append(v)
        else:
            raise KeyError(layout)
    return views


def _attn(g, B, T, L, mel_len, layout, ties=False, zero_pad=False):
    if ties:
        a = torch.randint(0, 4, (B, T, L), generator=g).float() * 0.25
    else:
        a = torch.softmax(torch.randn(B, T, L, generator=g) * 3.0, dim=-1)
    if zero_pad:
        a = a * (torch.arange(T)[None, :, None] < mel_len[:, None, None].cpu())
    a = a.to(DEV)
    if layout.startswith("pad"):
        buf = torch.full((B + 1, T + 2, L + (4 if layout == "pad_btc" else 3)), float("nan"), device=DEV)
        v = buf[1:, 1:T + 1, :L]
        v.copy_(a)
        return v
    return a.contiguous()


def _lengths(g, B, T, L, kind):
    ml = torch.randint(1, T + 1, (B,), generator=g)
    tl = torch.randint(1, L + 1, (B,), generator=g)
    ml[0] = T
    if kind == "ragged" and B > 1:
        ml[1] = 1
        tl[-1] = 1
    if kind == "full":
        ml[:] = T
    return ml.to(DEV), tl.to(DEV)


def _strides(x, C):
    return runtime._mel_strides(x, C)


def call(mel_out, mel_target, mel_len, text_len, attn, dct, ws_pad=7, out_pad=5):
    """The C entry with a NaN sentinel around out and the workspace -> (out [3], sentinels intact)."""
    B, T, L = attn.shape if attn is not None else (mel_len.shape[0], _strides(mel_out, dct.shape[0])[1], 0)
    C, n_mfcc = dct.shape if dct is not None else (0, 0)
    m = _strides(mel_out, C) if mel_out is not None else (None,) * 5
    t = _strides(mel_target, C) if mel_target is not None else (None,) * 5
    need = runtime.metrics_workspace_floats(B, T)
    ws = torch.full((need + 2 * ws_pad,), float("nan"), device=DEV)
    ob = torch.full((3 + 2 * out_pad,), float("nan"), device=DEV)
    rc = runtime.lib().ispk_acoustic_metrics_f32(
        runtime._ptr(mel_out), m[2], m[3], m[4], runtime._ptr(mel_target), t[2], t[3], t[4], mel_len.data_ptr(),
        runtime._ptr(text_len), runtime._ptr(attn), attn.stride(0) if attn is not None else 0,
        attn.stride(1) if attn is not None else 0, runtime._ptr(dct), ws[ws_pad:].data_ptr(), need,
        ob[out_pad:].data_ptr(), B, C, T, L, n_mfcc, runtime._stream())
    assert rc == 0, runtime.lib().ispk_last_error_string()
    torch.cuda.synchronize()
    intact = bool(torch.isnan(ws[:ws_pad]).all() and torch.isnan(ws[ws_pad + need:]).all() and torch.isnan(ob[:out_pad]).all()
                  and torch.isnan(ob[out_pad + 3:]).all())
    return ob[out_pad:out_pad + 3].clone(), intact


def check(mel_out, mel_target, mel_len, text_len, attn, dct):
    got, intact = call(mel_out, mel_target, mel_len, text_len, attn, dct)
    again, _ = call(mel_out, mel_target, mel_len, text_len, attn, dct)
    ref = ref64(mel_out, mel_target, mel_len, text_len, attn, dct)
    assert intact, "a store outside out / the workspace"
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)), "repeat call differs"
    g, r = got.double().cpu(), ref.cpu()
    assert torch.isfinite(g).all(), g
    T, B = attn.shape[1], attn.shape[0]
    nch = (T + 31) // 32
    len_tol = (32 + nch + math.ceil(B / 256) + 10) * EPS32 * abs(float(r[1])) + 1e-12
    assert abs(g[0] - r[0]) <= 1e-5 * abs(r[0]) + 1e-9, ("mcd", float(g[0]), float(r[0]))
    assert abs(g[1] - r[1]) <= len_tol, ("alignment_length", float(g[1]), float(r[1]), len_tol)
    assert abs(g[2] - r[2]) <= 1e-5 * abs(r[2]), ("alignment_strength", float(g[2]), float(r[2]))
    return got


# ---------------------------------------------------------------------------------------------------- the matrix
def _matrix():
    Bs, Ts, Ls = (1, 2, 5, 64, 65), (1, 2, 63, 64, 65, 512, 1723), (1, 3, 100, 101)
    layouts = ("bct", "btc", "pad_bct", "pad_btc", "mixed")
    cases, i = [], 0
    for T in Ts:
        for B in Bs:
            if B * T > 65 * 512 and B != 5:
                continue                      # (1723 frames at B = 1, 2, 5 only: the float64 side is the slow one)
            L = Ls[i % 4]
            cases.append((B, T, L, layouts[i % 5], 13 if i % 3 else 20, ("ragged", "random", "full")[i % 3], i % 4 == 1,
                          i % 2 == 0))
            i += 1
    for lay in layouts:                                             # every layout at chunk edges and both text-width paths
        for T, L in ((65, 100), (96, 101), (33, 3)):
            cases.append((5, T, L, lay, 13, "ragged", False, False))
    for B in (1, 2, 5, 64):                                         # the T == 80 quirk: [B, 80, 80] is read frames-first
        cases.append((B, 80, 17 if B % 2 else 100, "quirk", 13, "ragged", B == 5, True))
        cases.append((B, 80, 100, "quirk", 20, "full", False, False))
    for T in (31, 32, 33, 64, 65, 97, 1723):                        # ties everywhere, chunk boundaries included
        cases.append((3, T, 9, "bct", 13, "ragged", True, False))
        cases.append((2, T, 101, "btc", 13, "full", True, True))
    return cases


MATRIX = _matrix()


def _cid(c):
    B, T, L, lay, n, lk, ties, zp = c
    return f"B{B}-T{T}-L{L}-{lay}-m{n}-{lk}{'-ties' if ties else ''}{'-zpad' if zp else ''}"


@pytest.mark.parametrize("case", MATRIX, ids=[_cid(c) for c in MATRIX])
def test_metrics_matrix_against_float64(case):
    B, T, L, layout, n_mfcc, lkind, ties, zero_pad = case
    g = torch.Generator().manual_seed(zlib.crc32(_cid(case).encode()))
    C = 80
    ml, tl = _lengths(g, B, T, L, lkind)
    mo, mt = _mel_pair(g, B, C, T, layout, ml)
    attn = _attn(g, B, T, L, ml, layout, ties=ties, zero_pad=zero_pad)
    check(mo, mt, ml, tl, attn, create_dct(n_mfcc, C).to(DEV))


def test_ties_across_a_chunk_boundary_pick_the_first_index():
    """Rows 31 / 32 (the two sides of the first chunk edge) and 63 / 64 with ties whose LAST index would change every step."""
    B, T, L = 2, 96, 12
    attn = torch.zeros(B, T, L)
    for t in range(T):
        attn[:, t, t % 5] = 1.0
        attn[:, t, 11 - t % 3] = 1.0          # an equal maximum further right
    attn = attn.to(DEV)
    ml = torch.tensor([96, 70], device=DEV)
    tl = torch.tensor([12, 9], device=DEV)
    g = torch.Generator().manual_seed(1)
    mo, mt = _mel_pair(g, B, 80, T, "bct", ml)
    got = check(mo, mt, ml, tl, attn, create_dct(13, 80).to(DEV))
    steps = lambda a, n: sum(math.sqrt(1 + (a[t] - a[t - 1]) ** 2) for t in range(1, n))   # noqa: E731
    first = [t % 5 for t in range(T)]
    exp = (steps(first, 96) / math.hypot(12, 96) + steps(first, 70) / math.hypot(9, 70)) / 2
    assert abs(float(got[1]) - exp) < 1e-5 * exp


def test_nan_padding_is_never_read_and_layout_rule_matches_the_reference():
    """A [B, T, 80] pair and its [B, 80, T] transpose give the same bits; so do NaN-padded views of them."""
    g = torch.Generator().manual_seed(4)
    B, T, L = 5, 77, 23
    ml, tl = _lengths(g, B, T, L, "ragged")
    outs = []
    for lay in ("bct", "btc", "pad_bct", "pad_btc"):
        g2 = torch.Generator().manual_seed(9)
        mo, mt = _mel_pair(g2, B, 80, T, lay, ml)
        attn = _attn(torch.Generator().manual_seed(3), B, T, L, ml, lay)
        outs.append(call(mo, mt, ml, tl, attn, create_dct(13, 80).to(DEV))[0])
    for o in outs[1:]:
        assert torch.allclose(o, outs[0], rtol=1e-6, atol=0)
    assert all(torch.isfinite(o).all() for o in outs)


# ---------------------------------------------------------------------------------------------------- fixture: the reference
@pytest.mark.parametrize("case", list(synth.METRIC_CASES))
def test_metrics_against_the_reference_fixture(case):
    gld = golden("metrics.npz")
    d = synth.make_metric_inputs(case)
    assert [crc(d[k]) for k in ("mel_out", "mel_target", "attn_soft", "mel_len", "text_len")] == [int(v) for v in gld[f"{case}_crc"]]
    d = {k: v.to(DEV) for k, v in d.items()}
    ev = AcousticModelEvaluator(None)
    outputs = {"mel": d["mel_out"], "aligner_output": {"attn_soft": d["attn_soft"]}}
    m = ev({"mel": d["mel_target"], "mel_len": d["mel_len"], "text_len": d["text_len"]}, outputs)
    got = np.array([float(m[k]) for k in ("metrics/mcd_13", "metrics/alignment_length", "metrics/alignment_strength")])
    np.testing.assert_allclose(got, gld[f"{case}_values"].astype(np.float64), rtol=1e-5)


def test_metrics_of_the_models_forward_against_the_reference_fixture(gpu_model):
    """The reference evaluator on the reference model's own forward (B = 2, forward.npz's inputs) against this evaluator on
    this model's forward of the same inputs (the forwards agree to ~1e-5: tests/test_gpu_model.py)."""
    gld = golden("metrics.npz")
    inp = synth.make_inputs(2, 100, 512)
    text_len, mel_len = torch.tensor([100, 73]), torch.tensor([512, 390])
    tm = torch.arange(100)[None] < text_len[:, None]
    mm = torch.arange(512)[None] < mel_len[:, None]
    text, mel = inp["text"] * tm, inp["mel"] * mm[:, None]
    pitch, energy = inp["pitch"] * mm, inp["energy"] * mm
    assert [crc(t) for t in (text, mel, pitch, energy, mel_len, text_len)] == [int(v) for v in gld["forward_crc"]]
    args = [t.to(DEV) for t in (text, text_len, mel, mel_len, pitch, energy)]
    out = gpu_model(*args, flow_noise=inp["flow_x0"].to(DEV), flow_time=inp["flow_t"].to(DEV))
    m = AcousticModelEvaluator(gpu_model)({"mel": args[2], "mel_len": args[3], "text_len": args[1]}, out)
    got = np.array([float(m[k]) for k in ("metrics/mcd_13", "metrics/alignment_length", "metrics/alignment_strength")])
    np.testing.assert_allclose(got, gld["forward_values"].astype(np.float64), rtol=1e-4)


# ---------------------------------------------------------------------------------------------------- end to end
def _model(state_dict, train_mode):
    from isp_tts_amd.acoustic import AcousticModel
    from isp_tts_amd.config import AcousticDims
    m = AcousticModel.init(AcousticDims().model_config())
    m.load_state_dict(state_dict, strict=True)
    m = m.to(DEV)
    return m.train() if train_mode else m.eval()


def _collated(inp):
    return {"text_vector": inp["text"].to(DEV), "text_vector_len": inp["text_len"].to(DEV), "mel": inp["mel"].to(DEV),
            "mel_len": inp["mel_len"].to(DEV), "pitch": inp["pitch"].to(DEV), "energy": inp["energy"].to(DEV), "speaker": None,
            "filename": ["utt_0", "utt_1", "utt_2"]}


def _against_float64(metrics, inputs, outputs, evaluator):
    assert set(metrics) == {"metrics/mcd_13", "metrics/alignment_length", "metrics/alignment_strength"}
    vals = torch.stack([metrics[k] for k in ("metrics/mcd_13", "metrics/alignment_length", "metrics/alignment_strength")])
    assert all(v.dim() == 0 and v.dtype == torch.float32 and v.is_cuda for v in metrics.values())
    # one device buffer behind all three
    assert len({v.untyped_storage().data_ptr() for v in metrics.values()}) == 1
    ref = ref64(outputs.mel.detach(), inputs["mel"], inputs["mel_len"], inputs["text_len"],
                outputs.aligner_output.attn_soft.detach(), evaluator.mcd_evaluator.dct(DEV))
    g, r = vals.double(), ref
    assert abs(g[0] - r[0]) <= 1e-5 * abs(r[0])
    assert abs(g[1] - r[1]) <= 1e-6 * abs(r[1])
    assert abs(g[2] - r[2]) <= 1e-5 * abs(r[2])


@pytest.mark.parametrize("amp", [False, True])
def test_reference_loop_body_with_the_evaluator(state_dict, amp):
    """experiments/trainer.py:543-559: outputs = model(**inputs); loss = criterion(...); metrics = evaluator(inputs, outputs),
    against the float64 restatement on those outputs, then the step still trains (the evaluator leaves the tape alone)."""
    batch = _collated(synth.make_inputs(3, 52, 160, variable=True, seed=9))
    model = _model(state_dict, True)
    model.train_amp = amp
    criterion = train.AcousticModelLoss()
    optimizer = train.FlatAdamW(model.parameters(), lr=2e-4, weight_decay=1e-2, grad_clip=1.0)
    evaluator = AcousticModelEvaluator(model)
    torch.manual_seed(3)
    inputs = model.prepare_inputs(batch)
    outputs = model(**inputs)
    loss, losses = criterion(inputs=inputs, outputs=outputs, step=0)
    metrics = evaluator(inputs, outputs)
    assert outputs.mel.grad_fn is not None
    _against_float64(metrics, inputs, outputs, evaluator)
    norm = optimizer.step(loss)
    assert torch.isfinite(norm) and float(norm) > 0


def test_evaluation_forward_with_the_evaluator(state_dict):
    """trainer.py:534 evaluates under torch.no_grad(): the inference forward, the same evaluator call, and
    on_eval_epoch_end's two figures of item 0."""
    batch = _collated(synth.make_inputs(3, 52, 160, variable=True, seed=9))
    model = _model(state_dict, False)
    evaluator = AcousticModelEvaluator(model)
    with torch.no_grad():
        inputs = model.prepare_inputs(batch)
        outputs = model(**inputs)
        metrics = evaluator(inputs, outputs)
    _against_float64(metrics, inputs, outputs, evaluator)
    pytest.importorskip("matplotlib")
    from matplotlib.figure import Figure
    images = evaluator.on_eval_epoch_end(inputs=batch, outputs=outputs)
    assert set(images) == {"images/eval/alignment", "images/eval/mel_spectrogram"}
    assert all(isinstance(f, Figure) for f in images.values())
    ml, tl = int(batch["mel_len"][0]), int(batch["text_vector_len"][0])
    shapes = [tuple(ax.images[0].get_array().shape) for ax in images["images/eval/alignment"].axes if ax.images]
    assert shapes == [(tl, ml), (tl, ml)]
    spec = [ax.images[0].get_array() for ax in images["images/eval/mel_spectrogram"].axes if ax.images]
    target = batch["mel"][0, :, :ml].cpu().numpy()
    assert spec[0].shape == (80, ml) and np.array_equal(np.asarray(spec[0]), target)
    assert spec[1].min() >= target.min() and spec[1].max() <= target.max()


def test_mcd_and_alignment_metric_on_their_own():
    d = {k: v.to(DEV) for k, v in synth.make_metric_inputs("ragged").items()}
    both = AcousticModelEvaluator()({"mel": d["mel_target"], "mel_len": d["mel_len"], "text_len": d["text_len"]},
                                    {"mel": d["mel_out"], "aligner_output": {"attn_soft": d["attn_soft"]}})
    mcd = MCD()(d["mel_out"], d["mel_target"], d["mel_len"])
    length, strength = AlignmentMetric()(d["attn_soft"], d["mel_len"], d["text_len"])
    assert torch.equal(mcd, both["metrics/mcd_13"])
    assert torch.equal(length, both["metrics/alignment_length"]) and torch.equal(strength, both["metrics/alignment_strength"])
    m20 = MCD(n_mfcc=20)(d["mel_out"], d["mel_target"], d["mel_len"])
    ref = ref64(d["mel_out"], d["mel_target"], d["mel_len"], d["text_len"], d["attn_soft"], create_dct(20, 80).to(DEV))
    assert abs(float(m20) - float(ref[0])) <= 1e-5 * abs(float(ref[0]))


def test_evaluator_issues_no_aten_compute_ops():
    """The evaluator call is libispk launches only: the spy of test_gpu_train.py::test_training_step_issues_no_aten_compute_ops
    sees views and allocations on the device and nothing else."""
    from torch.utils._python_dispatch import TorchDispatchMode
    from torch.utils._pytree import tree_flatten
    harmless = ("aten.view", "aten.empty", "aten._unsafe_view", "aten.transpose", "aten.slice", "aten.select",
                "aten.unsqueeze", "aten.expand", "aten.detach", "aten.alias", "aten.t.", "aten.permute", "aten.squeeze",
                "aten.reshape", "aten.as_strided", "aten.is_", "aten.size", "aten.stride", "aten.lift_fresh",
                "aten._reshape_alias", "aten.split", "aten.unbind", "aten.sym_", "aten.empty_like", "aten.new_empty",
                "aten.record_stream", "aten.view_as")
    seen = []

    class Spy(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            out = func(*args, **(kwargs or {}))
            name = str(func)
            if not name.startswith(harmless):
                if any(t.is_cuda for t in tree_flatten((args, kwargs, out))[0] if isinstance(t, torch.Tensor)):
                    seen.append(name)
            return out

    d = {k: v.to(DEV) for k, v in synth.make_metric_inputs("ties").items()}
    ev = AcousticModelEvaluator()
    inputs = {"mel": d["mel_target"], "mel_len": d["mel_len"], "text_len": d["text_len"]}
    outputs = {"mel": d["mel_out"], "aligner_output": {"attn_soft": d["attn_soft"]}}
    ev(inputs, outputs)                       # (the first call puts the DCT basis on the device)
    torch.cuda.synchronize()
    with Spy():
        m = ev(inputs, outputs)
    torch.cuda.synchronize()
    assert seen == [], f"PyTorch kernels inside the evaluator: {sorted(set(seen))}"
    assert all(torch.isfinite(v) for v in m.values())


def test_graphed_step_reports_the_metrics(state_dict):
    """GraphedTrainStep(..., evaluator=): after each of two replays, step.metrics equals bit for bit the eager evaluator on
    step.outputs; a step built without the evaluator gives the same losses and norm."""
    d = {k: v.to(DEV) for k, v in synth.make_inputs(3, 52, 160, variable=True, seed=9).items()}
    batch = {k: d[k] for k in ("text", "text_len", "mel", "mel_len", "pitch", "energy", "flow_x0", "flow_t")}

    def run(evaluator):
        torch.manual_seed(21)
        m = _model(state_dict, False)
        o = train.FlatAdamW(m.parameters(), lr=1e-3, weight_decay=1e-2, grad_clip=1.0)
        step = train.GraphedTrainStep(m, o, batch, amp=True, evaluator=evaluator)
        res = []
        for _ in range(2):
            total, losses, norm = step()
            torch.cuda.synchronize()
            rec = [total.clone(), {k: v.clone() for k, v in losses.items()}, norm.clone()]
            if evaluator is not None:
                eager = evaluator({k: batch[k] for k in ("mel", "mel_len", "text_len")}, step.outputs)
                for k, v in step.metrics.items():
                    assert torch.equal(v, eager[k]), k
                    assert torch.isfinite(v)
                rec.append({k: v.clone() for k, v in step.metrics.items()})
            res.append(rec)
        assert res[0][-1] is not None
        step.close()
        return res

    with_ev = run(AcousticModelEvaluator())
    without = run(None)
    for a, b in zip(with_ev, without):
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
        assert all(torch.equal(a[1][k], b[1][k]) for k in b[1])
    assert not torch.equal(with_ev[0][3]["metrics/mcd_13"], with_ev[1][3]["metrics/mcd_13"])   # (the replays trained)


# ---------------------------------------------------------------------------------------------------- refusals, B = 0
def test_refusals_leave_out_untouched():
    lib = runtime.lib()
    dev = lambda *s: torch.zeros(*s, device=DEV)       # noqa: E731
    mel = dev(2, 80, 40)
    attn = dev(2, 40, 10)
    ml = torch.full((2,), 40, dtype=torch.int64, device=DEV)
    dct = create_dct(13, 80).to(DEV)
    ws = dev(1000)
    out = torch.full((3,), 7.0, device=DEV)
    P = lambda t: t.data_ptr() if t is not None else None   # noqa: E731

    def rc(mo=mel, mt=mel, lens=ml, tl=ml, at=attn, dc=dct, w=ws, wn=1000, o=out, B=2, C=80, T=40, L=10, n=13):
        r = lib.ispk_acoustic_metrics_f32(P(mo), 3200, 40, 1, P(mt), 3200, 40, 1, P(lens), P(tl), P(at), 400, 10, P(dc), P(w), wn,
                                          P(o), B, C, T, L, n, None)
        return r, lib.ispk_last_error_string()

    assert rc(lens=None)[0] == -1 and rc(o=None)[0] == -1 and rc(w=None)[0] == -1
    assert rc(mo=None)[0] == -1 and rc(dc=None)[0] == -1 and rc(mo=None, mt=None, at=None)[0] == -1
    assert rc(tl=None)[0] == -1
    assert rc(B=0)[0] == -2 and rc(T=0)[0] == -2 and rc(L=0)[0] == -2 and rc(B=65536)[0] == -2
    assert rc(n=81)[0] == -2 and rc(n=0)[0] == -2
    r, msg = rc(C=129, n=13)
    assert r == -2 and b"128" in msg
    assert rc(wn=2 * 3 - 1)[0] == -3
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full((3,), 7.0, device=DEV))
    # the lengths are device data: mel_len < 1 (or > T) cannot be refused by the return code and makes the outputs NaN
    bad = torch.tensor([40, 0], dtype=torch.int64, device=DEV)
    assert rc(lens=bad)[0] == 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


def test_empty_batch_through_the_wrapper():
    """B = 0: the reference's means over an empty batch are 0 / 0 - NaN for all three, without a launch."""
    e = torch.zeros(0, 80, 7, device=DEV)
    ml = torch.zeros(0, dtype=torch.int64, device=DEV)
    out = runtime.acoustic_metrics(e, e, ml, ml, torch.zeros(0, 7, 5, device=DEV), create_dct(13, 80).to(DEV))
    assert out.shape == (3,) and torch.isnan(out).all()
    m = AcousticModelEvaluator()({"mel": e, "mel_len": ml, "text_len": ml},
                                 {"mel": e, "aligner_output": {"attn_soft": torch.zeros(0, 7, 5, device=DEV)}})
    assert all(torch.isnan(v) for v in m.values())
