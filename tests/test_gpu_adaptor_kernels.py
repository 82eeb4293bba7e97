"""The adaptor and between-stack kernels (csrc/glue.hip, the non-aligner half of csrc/aligner.hip), each against its float64
reference (tests/adaptor_reference.py, proved against the oracle and plain PyTorch expressions by
tests/test_adaptor_reference_host.py), through the `runtime` wrappers, at the smallest shapes that reach every branch.  Every test
runs its kernel twice on the same inputs (same bits) and checks that the inputs are unchanged.

Branches per entry point
  ispk_length_regulate_f32 / _split_bf16 / _split_f16 (length_regulate_body<D / 128, 0 | 1 | 2, false>; a workgroup owns 64 frames,
  the token axis streams in chunks of 16, the next chunk is fetched while the current one multiplies)      (B, M, L, D)
    (2, 1, 1, 256)     <2>; M = 1 < 64, L = 1 < 16: one frame and one token live, no prefetch; max_len -1 with the sum (3) above M:
                       mask all ones, dec_len unclamped; utterance 1 has only zero durations (dec_len 0); enc_len (1, 0)
    (1, 63, 15, 256)   <2>; M = 63, L = 15: one short of the tile and of the chunk; max_len 40 below the sum and below M (the
                       clamped dec_len cuts the soft path); enc_len 9 with non-zero durations behind it; x row-strided (ldx = D + 16)
    (2, 64, 16, 256)   <2>; M == 64, L == 16: exactly one tile and one chunk, no trailing prefetch; max_len = M clamps utterance 0;
                       enc_len (16, 0): utterance 1 has dec_len > 0 and no weight at all
    (3, 65, 17, 384)   <3>; a second tile of one frame, a second chunk of one token; max_len -1, sums above M / 0 / below M;
                       enc_len (17, 0, 16): token 16, alone in its chunk, is masked and has a non-zero duration
    (2, 128, 48, 384)  <3>; two full tiles, three full chunks (L a multiple of 16); max_len 100 below the sum and below M; enc_len
                       (48, 0); x row-strided
    (2, 130, 33, 384)  <3>; a third tile of two frames, a third chunk of one token; max_len = M clamps utterance 0; enc_len (0, 33)
    modes: an alignment with int64 [B, L] / int64 [B, 1] / fp32 [B, L] durations (the last: dur_f32 together with an alignment),
    the soft path without and with enc_len.  Exact inputs (integers, durations in quarters): all three entry points must equal
    float64 exactly, so a mis-indexed or dropped token, chunk, tile or feature column shows whatever its weight.  Then once more
    with softmax alignments and normal x: fp32 and split-f16 at the measured tolerance, split-bf16 within 2^-16 (|A| @ |x|) of it.
  ispk_soft_average_f32 (16 frame lanes x 64 text columns; the eight-fold trip runs while a lane's frame + 112 < M)   (B, M, L)
    (2, 1, 1)     lane 0 alone has a frame; one column       (2, 15, 5)    15 lanes, one frame each, tail loop only
    (3, 17, 65)   lane 0 takes two tail frames; L > 64: a second column block of one column
    (2, 112, 64)  mm + 112 < M fails for every lane: tail loop only, 7 frames per lane; L == 64: one full block
    (2, 113, 63)  lane 0 alone takes the eight-fold trip (and nothing after it), lanes 1 .. 15 the tail loop
    (2, 129, 64)  every lane takes the trip; the tail is frame 128 alone (lane 0)
    (1, 300, 130) two trips per lane, then 2 or 3 tail frames; three column blocks, the last of two columns
    each with duration None (column 0 written as 0) and int64 durations with zeros; text_len with 0 and L; one text column whose
    attention is 0 in every frame (its targets are exactly 0 / 1e-5 = 0)
  ispk_flow_mix_f32: the shapes of FLOW_FINISH_CASES, t with exact 0 and 1; bit-exact
  ispk_flow_finish_f32 (one workgroup, 16 lanes per utterance, 64 utterances per pass)                      (B, L, C)
    (1, 1, 1)     L * C = 1 < 16: lane 0 alone has an element     (3, 5, 1), (2, 6, 3)   L * C = 5 < 16, 18: one lane takes two
    (5, 37, 3)    111 elements, 7 per lane                         (70, 37, 3)  a second pass of 6 utterances
    (1100, 2, 3)  B > 1024: 18 passes, thread 0 reads ratio[] back from global memory instead of LDS
    lengths include 0 (the ratio's denominator is max(0, 1e-5): exactly 0) and L
  ispk_flow_head_f32 (flow_head_kernel: 16 rows per workgroup, 4 per wave; flow_head_finalize_kernel: 1024 utterances per trip)  (B, L)
    (1, 1)   L < 4: one live row, three clamped ones     (2, 3)   L < 4; lengths (3, 0): an utterance with no valid row
    (3, 16)  L a multiple of 16: no clamped row          (2, 17)  a second block of one row; y a column slice (ldy = 264 > 256)
    (5, 37)  three blocks; the masked rows of y hold NaN: no output may be NaN, masked pred and duration are exactly 0
    (1030, 2) the finalizer's second trip (6 utterances)
  ispk_flow_euler_f32: (1, 1, 1), (5, 37, 3), (3, 100, 3) = 1, 555, 900 elements (1, 3, 4 workgroups); mask None / lengths with 0;
    dt 0.125 (exact in fp32) and 0.1; bit-exact
  ispk_infer_features_f32 / _round_f32 (infer_features_kernel<false | true>; one thread per token)          (B, L)
    (1, 1), (3, 37), (2, 300) = 1, 111, 600 tokens (1, 1, 3 workgroups); no target / fp32 duration target with a third of its
    entries negative / int64 duration target with -1 entries (both with zeros: `>= 0` replaces) / pitch target / energy target /
    both; default factors and (1.3, 0.9, 0.25, 1.1, -0.5); round_duration off and on
  ispk_time_embedding_f32 (one wave per time value, lane j < E owns hidden unit j and output j)             (n, H, E)
    (1, 32, 32), (67, 32, 32) the model's sizes     (5, 1, 1) one frequency, one live lane     (3, 64, 64) the documented limits
    (4, 7, 33) sizes that are multiples of nothing  (0, 32, 32) no launch
  ispk_embed_tokens_f32 (one wave per token row, 4 rows per workgroup, D / 4 float4 over 64 lanes)          (V, D, B, L)
    (149, 384, 5, 77)  385 rows: the last workgroup has one      (3, 4, 1, 1)  D = 4: lane 0 alone copies
    (10, 260, 3, 2)    6 rows end a workgroup half-way; D / 4 = 65: lane 0 takes a second float4; the table a column slice
    (ld_table = D + 8); text_len with 0; ids -1, V and 2^40 read row 0

Tolerances.  Exact where the arithmetic is exact (see above, and adaptor_reference's docstring).  Otherwise max |diff| / max |ref|:
the same formula evaluated in fp32 torch on the CPU at every case above loses the figure below against float64 (max over the
cases; re-measured and printed per case by test_adaptor_reference_host.py::test_fp32_noise_table), and the kernel is allowed
8 x that, capped at 1e-4.

    output                       fp32 noise   tolerance
    length_regulate out          2.755e-7     2.20e-6      (fp32 and split-f16 entries; split-bf16: + 2^-16 (|A| @ |x|) per element)
    soft_average log_duration    2.718e-8     2.17e-7
    soft_average targets         5.845e-7     4.68e-6
    flow_head pred               3.369e-7     2.70e-6
    flow_head duration           6.043e-7     4.83e-6
    flow_head ratio              2.955e-7     2.36e-6
    flow_head loss               1.697e-7     1.36e-6
    flow_finish duration         2.198e-7     1.76e-6
    flow_finish ratio            9.089e-8     7.27e-7
    flow_finish loss             5.613e-8     4.49e-7
    infer_features duration      2.841e-7     2.27e-6      (the predicted ones; those taken from a target are exact)
    time_embedding out           2.849e-7     2.28e-6
"""
import pytest
import torch

import adaptor_reference as R
from isp_tts_amd import runtime

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32


def _dev(t):
    return None if t is None else t.to(DEV)


def _unchanged(pairs):
    for name, d, h in pairs:
        assert d is None or R.same_bits(d, h), f"{name} was written"


def _same_bits(a, b) -> bool:
    """R.same_bits, 0-d tensors (the loss) included."""
    return a.shape == b.shape and R.same_bits(a.reshape(-1), b.reshape(-1))


def _max0(t) -> float:
    return float(t.abs().max()) if t.numel() else 0.0


# ------------------------------------------------------------------------------------------------ length_regulate


def _lr_run(i, D, split):
    """-> (run, inputs): run() calls the wrapper on device copies made once; inputs = [(name, device tensor, host tensor)]."""
    wide = _dev(i["wide"])
    x = wide[:, :, 8:8 + D] if wide is not None else i["x"].to(DEV)
    dur, A, enc = i["dur"].to(DEV), _dev(i["alignment"]), _dev(i["enc_len"])
    if wide is not None:
        assert x.stride(1) == D + 16          # the wrapper passes ldx = D + 16, no copy

    def run():
        return [t.cpu() for t in runtime.length_regulate(x, dur, A, i["M"], max_len=i["max_len"], enc_len=enc, split_bf16=split)]
    held = [("x", wide if wide is not None else x, i["wide"] if wide is not None else i["x"]), ("durations", dur, i["dur"]),
            ("alignment", A, i["alignment"]), ("enc_len", enc, i["enc_len"])]
    return run, held


@pytest.mark.parametrize("entry,split", R.LR_ENTRIES)
@pytest.mark.parametrize("mode", R.LR_MODES)
@pytest.mark.parametrize("case", R.LR_CASES)
def test_length_regulate_exact(case, mode, entry, split):
    B, M, L, D = case
    i = R.lr_inputs(case, mode)
    want, want_dl, want_mask = R.length_regulate_ref(i["x"], i["dur"], i["alignment"], M, i["max_len"], i["enc_len"])
    run, held = _lr_run(i, D, split)
    out, dl, mask = run()
    assert out.shape == (B, M, D) and out.dtype == F32 and dl.dtype == torch.int64 and mask.dtype == torch.bool
    assert torch.equal(dl, want_dl), f"dec_len {dl.tolist()} vs {want_dl.tolist()}"
    assert torch.equal(mask, want_mask)
    wrong = out.double() != want
    assert not bool(wrong.any()), f"{int(wrong.sum())} values differ, first at {wrong.nonzero()[0].tolist()}"
    if i["alignment"] is None:
        for b in range(B):
            assert _max0(out[b, int(dl[b]):]) == 0.0
            if int(dl[b]) == 0 or (i["enc_len"] is not None and int(i["enc_len"][b]) == 0):
                assert _max0(out[b]) == 0.0
    for a, b in zip(run(), (out, dl, mask)):
        assert R.same_bits(a, b)
    _unchanged(held)


@pytest.mark.parametrize("entry,split", R.LR_ENTRIES)
@pytest.mark.parametrize("case", R.LR_CASES)
def test_length_regulate_rounded_operands(case, entry, split):
    B, M, L, D = case
    i = R.lr_inputs(case, "align_i64", exact=False)
    want, want_dl, want_mask = R.length_regulate_ref(i["x"], i["dur"], i["alignment"], M, i["max_len"], None)
    run, held = _lr_run(i, D, split)
    out, dl, mask = run()
    assert torch.equal(dl, want_dl) and torch.equal(mask, want_mask)
    tol = R.tol("length_regulate.out")
    err = (out.double() - want).abs()
    print(f"{case} {entry}: max |diff| / max |ref| = {R.rel_err(out, want):.3e} (fp32 tolerance {tol:.3g})")
    if entry == "split_bf16":
        bound = R.lr_bf16_bound(i["alignment"], i["x"]) + tol * float(want.abs().max())
        print(f"    worst |diff| / bound = {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), f"worst |diff| / bound = {float((err / bound).max()):.3f}"
    else:
        R.close(out, want, tol, "out")
    for a, b in zip(run(), (out, dl, mask)):
        assert R.same_bits(a, b)
    _unchanged(held)


# ------------------------------------------------------------------------------------------------ soft_average


@pytest.mark.parametrize("with_duration", [False, True])
@pytest.mark.parametrize("case", R.SA_CASES)
def test_soft_average(case, with_duration):
    B, M, L = case
    i = R.sa_inputs(case)
    dur = i["duration"] if with_duration else None
    want = R.soft_average_ref(i["attn"], i["pitch"], i["energy"], dur, i["text_len"])
    d = {k: _dev(i[k]) for k in ("attn", "pitch", "energy", "text_len")}
    dd = _dev(dur)
    run = lambda: runtime.soft_average(d["attn"], d["pitch"], d["energy"], dd, d["text_len"]).cpu()      # noqa: E731
    got = run()
    assert got.shape == (B, L, 3) and got.dtype == F32
    print(f"{case}: log_duration {R.rel_err(got[..., 0], want[..., 0]):.3e}, targets {R.rel_err(got[..., 1:], want[..., 1:]):.3e}")
    if with_duration:
        R.close(got[..., 0], want[..., 0], R.tol("soft_average.log_duration"), "log1p(duration)")
        assert _max0(got[..., 0][i["duration"] == 0]) == 0.0
    else:
        assert _max0(got[..., 0]) == 0.0
    R.close(got[..., 1:], want[..., 1:], R.tol("soft_average.targets"), "pitch / energy targets")
    outside = torch.arange(L)[None] >= i["text_len"][:, None]
    assert _max0(got[..., 1:][outside]) == 0.0
    if i["zero_col"] is not None:
        assert _max0(got[:, i["zero_col"], 1:]) == 0.0
    assert R.same_bits(run(), got)
    _unchanged([(k, d[k], i[k]) for k in d] + [("duration", dd, dur)])


# ------------------------------------------------------------------------------------------------ flow_mix, flow_finish, flow_head


@pytest.mark.parametrize("case", R.FLOW_FINISH_CASES)
def test_flow_mix(case):
    i = R.flow_mix_inputs(case)
    want = R.flow_mix_ref(**i, dtype=F32)
    d = {k: i[k].to(DEV) for k in ("x0", "x1", "t")}
    run = lambda: [t.cpu() for t in runtime.flow_mix(d["x0"], d["x1"], d["t"], i["sigma"])]      # noqa: E731
    got = run()
    for name, g, w in zip(("x_t", "flow"), got, want):
        assert g.dtype == F32 and torch.equal(g, w), f"{name}: {int((g != w).sum())} values differ from the fp32 expression"
    for a, b in zip(run(), got):
        assert R.same_bits(a, b)
    _unchanged([(k, d[k], i[k]) for k in d])


def _check_flow_outputs(kernel, got, want, mask, exact_pred=None):
    pred, dur, ratio, loss = got
    B, L, C = pred.shape
    assert dur.shape == (B, L) and ratio.shape == (B,) and loss.shape == () and all(t.dtype == F32 for t in got)
    for name, g, w in zip(("pred", "duration", "ratio", "loss"), got, want):
        print(f"    {kernel}.{name}: {R.rel_err(g, w):.3e}")
    for name, g, w in zip(("pred", "duration", "ratio", "loss"), got, want):
        assert bool(torch.isfinite(g).all()), f"{name} is not finite"
        if name == "pred" and exact_pred is not None:
            assert torch.equal(g, exact_pred), f"pred: {int((g != exact_pred).sum())} values differ from the fp32 expression"
        else:
            R.close(g, w, R.tol(f"{kernel}.{name}"), name)
    assert _max0(pred[~mask]) == 0.0 and _max0(dur[~mask]) == 0.0
    assert _max0(ratio[mask.sum(1) == 0]) == 0.0


@pytest.mark.parametrize("case", R.FLOW_FINISH_CASES)
def test_flow_finish(case):
    i = R.flow_finish_inputs(case)
    want = R.flow_finish_ref(**i)
    d = {k: i[k].to(DEV) for k in i}
    run = lambda: [t.cpu() for t in runtime.flow_finish(d["raw"], d["flow"], d["x0"], d["mask"])]      # noqa: E731
    got = run()
    print(f"{case}")
    _check_flow_outputs("flow_finish", got, want, i["mask"], exact_pred=R.flow_finish_ref(**i, dtype=F32)[0])
    for a, b in zip(run(), got):
        assert _same_bits(a, b)
    _unchanged([(k, d[k], i[k]) for k in d])


@pytest.mark.parametrize("case", R.FLOW_HEAD_CASES)
def test_flow_head(case):
    i = R.flow_head_inputs(case)
    wide_h = i.pop("wide")
    want = R.flow_head_ref(**i)
    d = {k: i[k].to(DEV) for k in i if k not in ("y", "eps")}
    wide = _dev(wide_h)
    y = wide[:, :, 4:260] if wide is not None else i["y"].to(DEV)
    if wide is not None:
        assert y.stride(1) == 264
    run = lambda: [t.cpu() for t in runtime.flow_head(y, d["gamma"], d["beta"], i["eps"], d["W"], d["bias"], d["flow"],      # noqa: E731
                                                      d["x0"], d["mask"])]
    got = run()
    print(f"{case}")
    _check_flow_outputs("flow_head", got, want, i["mask"])
    for a, b in zip(run(), got):
        assert _same_bits(a, b)
    _unchanged([(k, d[k], i[k]) for k in d] + [("y", wide if wide is not None else y, wide_h if wide is not None else i["y"])])


# ------------------------------------------------------------------------------------------------ flow_euler, infer_features


@pytest.mark.parametrize("dt", R.FLOW_EULER_DT)
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("case", R.FLOW_EULER_CASES)
def test_flow_euler(case, masked, dt):
    i = R.flow_euler_inputs(case, masked)
    want = R.flow_euler_ref(i["x_t"], i["velocity"], dt, i["mask"], dtype=F32)
    d = {k: _dev(v) for k, v in i.items()}
    run = lambda: runtime.flow_euler(d["x_t"], d["velocity"], dt, d["mask"]).cpu()      # noqa: E731
    got = run()
    assert got.dtype == F32 and torch.equal(got, want), f"{int((got != want).sum())} values differ from the fp32 expression"
    R.close(got, R.flow_euler_ref(i["x_t"], i["velocity"], dt, i["mask"]), 1e-6, "against float64")
    if masked:
        assert _max0(got[~i["mask"]]) == 0.0
    assert R.same_bits(run(), got)
    _unchanged([(k, d[k], i[k]) for k in d])


@pytest.mark.parametrize("rnd", [False, True])
@pytest.mark.parametrize("fname", list(R.INFER_FACTORS))
@pytest.mark.parametrize("targets", R.INFER_TARGETS)
@pytest.mark.parametrize("case", R.INFER_CASES)
def test_infer_features(case, targets, fname, rnd):
    B, L = case
    i, fac = R.infer_inputs(case, targets), R.INFER_FACTORS[fname]
    want_d, _ = R.infer_features_ref(**i, **fac, round_duration=rnd)
    d32, f32 = R.infer_features_ref(**i, **fac, round_duration=rnd, dtype=F32)
    d = {k: _dev(v) for k, v in i.items()}
    run = lambda: [t.cpu() for t in runtime.infer_features(d["pred"], d["duration_target"], d["pitch_target"],      # noqa: E731
                                                           d["energy_target"], **fac, round_duration=rnd)]
    dur, feats = run()
    assert dur.shape == (B, L) and feats.shape == (B, L, 2) and dur.dtype == feats.dtype == F32
    assert torch.equal(feats, f32), f"features: {int((feats != f32).sum())} values differ from the fp32 expression"
    print(f"{case} {targets} {fname} round={rnd}: duration {R.rel_err(dur, want_d):.3e}")
    R.close(dur, want_d, R.tol("infer_features.duration"), "duration")
    if i["duration_target"] is not None:
        given = i["duration_target"] >= 0
        assert torch.equal(dur[given], i["duration_target"][given].float()), "a duration taken from the target is not the target"
        assert torch.equal(dur[given], d32[given])
    assert float(dur.min()) >= 0.0
    for a, b in zip(run(), (dur, feats)):
        assert R.same_bits(a, b)
    _unchanged([(k, d[k], i[k]) for k in d])


# ------------------------------------------------------------------------------------------------ time_embedding, embed_tokens


@pytest.mark.parametrize("n,H,E", R.TIME_FWD_SHAPES)
def test_time_embedding(n, H, E):
    i = R.time_fwd_inputs(n, H, E)
    want = R.time_embedding_ref(**i)
    d = {k: v.to(DEV) for k, v in i.items()}
    run = lambda: runtime.time_embedding(**d).cpu()      # noqa: E731
    got = run()
    assert got.shape == (n, E) and got.dtype == F32
    print(f"{(n, H, E)}: {R.rel_err(got, want):.3e}")
    R.close(got, want, R.tol("time_embedding.out"), "out")
    assert R.same_bits(run(), got)
    _unchanged([(k, d[k], i[k]) for k in d])


@pytest.mark.parametrize("case", R.EMBED_CASES)
def test_embed_tokens(case):
    V, D, B, L = case
    i = R.embed_inputs(case)
    want, want_mask = R.embed_tokens_ref(i["text"], i["table"], i["text_len"], dtype=F32)
    wide = _dev(i["wide"])
    table = wide[:, 4:4 + D] if wide is not None else i["table"].to(DEV)
    if wide is not None:
        assert table.stride(0) == D + 8
    text, text_len = i["text"].to(DEV), i["text_len"].to(DEV)
    run = lambda: [t.cpu() for t in runtime.embed_tokens(text, table, text_len)]      # noqa: E731
    emb, mask = run()
    assert emb.shape == (B, L, D) and emb.dtype == F32 and mask.dtype == torch.bool
    assert torch.equal(emb, want) and torch.equal(mask, want_mask)
    if i["bad"]:
        assert torch.equal(emb.reshape(-1, D)[i["bad"]], i["table"][0].expand(3, D)), "an id outside [0, V) did not read row 0"
    for a, b in zip(run(), (emb, mask)):
        assert R.same_bits(a, b)
    emb2, none = runtime.embed_tokens(text, table, None, want_mask=False)
    assert none is None and R.same_bits(emb2, emb)
    assert bool(runtime.embed_tokens(text, table, None)[1].all())
    _unchanged([("text", text, i["text"]), ("text_len", text_len, i["text_len"]),
                ("table", wide if wide is not None else table, i["wide"] if wide is not None else i["table"])])


# ------------------------------------------------------------------------------------------------ empty batches


def _empty(shape, dtype=F32):
    return torch.empty(shape, dtype=dtype, device=DEV)


def _is(t, shape, dtype=F32):
    return t.is_cuda and tuple(t.shape) == tuple(shape) and t.dtype == dtype


def test_an_empty_batch_returns_empty_tensors():
    i64, boo = torch.int64, torch.bool
    for split in (False, True, "f16"):
        out, dl, mask = runtime.length_regulate(_empty((0, 5, 256)), _empty((0, 5), i64), _empty((0, 7, 5)), 7, max_len=7, split_bf16=split)
        assert _is(out, (0, 7, 256)) and _is(dl, (0,), i64) and _is(mask, (0, 7), boo)
        out, dl, mask = runtime.length_regulate(_empty((0, 5, 384)), _empty((0, 5)), None, 7, enc_len=_empty((0,), i64), split_bf16=split)
        assert _is(out, (0, 7, 384)) and _is(dl, (0,), i64) and _is(mask, (0, 7), boo)
    assert _is(runtime.soft_average(_empty((0, 9, 5)), _empty((0, 9)), _empty((0, 9)), _empty((0, 5), i64), _empty((0,), i64)), (0, 5, 3))
    assert _is(runtime.soft_average(_empty((0, 9, 5)), _empty((0, 9)), _empty((0, 9)), None, _empty((0,), i64)), (0, 5, 3))
    xt, flow = runtime.flow_mix(_empty((0, 5, 3)), _empty((0, 5, 3)), _empty((0,)), 1e-5)
    assert _is(xt, (0, 5, 3)) and _is(flow, (0, 5, 3))
    for got in (runtime.flow_finish(_empty((0, 5, 3)), _empty((0, 5, 3)), _empty((0, 5, 3)), _empty((0, 5), boo)),
                runtime.flow_head(_empty((0, 5, 256)), _empty((256,)), _empty((256,)), 1e-5, _empty((3, 256)), _empty((3,)),
                                  _empty((0, 5, 3)), _empty((0, 5, 3)), _empty((0, 5), boo))):
        pred, dur, ratio, loss = got
        assert _is(pred, (0, 5, 3)) and _is(dur, (0, 5)) and _is(ratio, (0,)) and _is(loss, ())
    assert _is(runtime.flow_euler(_empty((0, 5, 3)), _empty((0, 5, 3)), 0.1), (0, 5, 3))
    assert _is(runtime.flow_euler(_empty((0, 5, 3)), _empty((0, 5, 3)), 0.1, _empty((0, 5), boo)), (0, 5, 3))
    for rnd in (False, True):
        dur, feats = runtime.infer_features(_empty((0, 5, 3)), _empty((0, 5), i64), _empty((0, 5)), None, round_duration=rnd)
        assert _is(dur, (0, 5)) and _is(feats, (0, 5, 2))
    emb, mask = runtime.embed_tokens(_empty((0, 5), i64), torch.ones((7, 8), device=DEV), _empty((0,), i64))
    assert _is(emb, (0, 5, 8)) and _is(mask, (0, 5), boo)
    i = {k: v.to(DEV) for k, v in R.time_fwd_inputs(0, 32, 32).items()}
    assert _is(runtime.time_embedding(**i), (0, 32))
    i["t"] = i["t"].view(0, 1)
    assert _is(runtime.time_embedding(**i), (0, 1, 32))
