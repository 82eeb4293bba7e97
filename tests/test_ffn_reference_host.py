"""The float64 references of tests/ffn_reference.py against plain PyTorch expressions, the rounding figures from which
tests/test_gpu_ffn_kernels.py takes its bound (every one under the ceiling of the older tests, and above zero where a value is
kept), the mutants - deliberately wrong references that the case tables must tell from the true one AT THE BOUND - the
restatement of the four-wave kernel's dispatch against a hand-written list of its instances, and the argument checks of the
feed-forward entry points that tests/test_ffn2_args_host.py does not cover.  CPU only.

The mutant table (mutant x entry -> the first killing case and the ratio of its worst figure to the bound) is printed by
test_every_mutant_is_killed_for_every_entry; a mutant that survives an entry it applies to fails that test.

Argument checks: as in test_ffn2_args_host.py every case breaks one condition of an otherwise valid call with `rows == 0` and
never-dereferenced pointers.  Two limits of that method, on purpose not worked around: ispk_ffn_bf16 / _prenorm look at ldw1 ==
dim, the weight size and the LayerNorm operands only after their `rows == 0` return, and the three staging entries have no
row count - a valid call launches - so only their refusals are pinned here (tests/test_gpu_ffn_kernels.py runs them).
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import ffn_reference as R
from isp_tts_amd import runtime

F64 = torch.float64
TOL = 1e-12
CASES = R.all_cases()


def entry_key(c):
    """The entry points as the issue lists them."""
    if c.entry == "attn_out_ffn":
        for v in ("stats", "norm_f32", "norm_bf16", "qkv"):
            if c.has(v):
                return f"attn_out_ffn+{v}"
    return c.entry


ENTRY_KEYS = sorted({entry_key(c) for c in CASES})


# ------------------------------------------------------------------------------------------------ references


def _torch_expr(c):
    """The entry's formula in PyTorch's own operators, float64."""
    i = {k: v.double() for k, v in R.inputs(c.dim, c.inner).items()}
    n, D = c.R, c.dim
    mask = R.mask_pattern(c.mask, n)
    zero = torch.zeros((), dtype=F64)

    def keep(v):
        return v if mask is None else torch.where(mask[:, None], v, zero)

    x, res = i["x"][:n], {}
    if c.entry == "ffn_fused":
        v = F.linear(F.gelu(F.linear(i["xb"][:n], i["w1"], i["bias1"] if c.has("bias1") else None)), i["w2"], i["bias2"] if c.has("bias2") else None)
        if c.flags & R.MASK_ACC:
            v = keep(v)
        if not c.has("noresid"):
            v = v + i["resid"][:n]
        out = keep(v) if c.flags & R.MASK_OUT else v
    else:
        proj = c.entry in R.PROJ_ENTRIES
        x1 = x
        if proj:
            o = i["o"][:n]
            x1 = x + F.linear(keep(o) if c.flags & R.MASK_ACC else o, i["wo"])
        h = F.layer_norm(x1, (D,), i["g"], i["b"], R.EPS)
        if c.entry in R.SPLIT_ENTRIES:
            k = c.inner // c.splits
            parts = [F.linear(F.gelu(F.linear(h, i["w1"][s * k:(s + 1) * k])), i["w2"][:, s * k:(s + 1) * k]) for s in range(c.splits)]
            if proj:
                parts[0] = parts[0] + x1
            res["parts"] = torch.stack(parts)
            out = keep(sum(parts) if proj else x + sum(parts))
        else:
            v = F.linear(F.gelu(F.linear(h, i["w1"])), i["w2"], i["bias2"] if c.has("bias2") else None)
            if c.flags & R.MASK_ACC and not proj:
                v = keep(v)
            v = v + x1
            out = keep(v) if c.flags & R.MASK_OUT else v
    res["y" if c.entry in R.SPLIT_ENTRIES else "out"] = out
    if c.has("stats"):
        res["stats"] = torch.stack([out.mean(1), 1.0 / torch.sqrt(out.var(1, unbiased=False) + R.EPS)], 1)
    if c.has("norm_f32") or c.has("norm_bf16"):
        ln = F.layer_norm(out, (D,), i["fg"], i["fb"], R.EPS)
        res["ln"] = keep(ln) if c.has("ln_mask") else ln
    if c.has("qkv"):
        res["qkv"] = F.linear(F.layer_norm(out, (D,), i["fg"], i["fb"], R.EPS), i["wq"])
    return res


@pytest.mark.parametrize("key", ENTRY_KEYS)
def test_exact_equals_plain_pytorch(key):
    """F.layer_norm -> F.linear -> F.gelu -> F.linear + residual with torch.where masks, to 1e-12 of the largest value."""
    n = 0
    for c in CASES:
        if entry_key(c) != key or c.inner > 192:
            continue
        got, want = R.evaluate(c), _torch_expr(c)
        assert set(got) == set(want), c.label
        for k in got:
            assert got[k].dtype == F64 and got[k].shape == want[k].shape
            scale = max(float(want[k].abs().max()), 1.0)
            assert float((got[k] - want[k]).abs().max()) <= TOL * scale, f"{c.label} {k}"
        n += 1
    assert n >= 5, key


def test_inputs_hold_the_conditions():
    """Weights are bf16 values; a case's rows are the first rows of one set; the constant row; every mask pattern has what its
    name says (and `prefix` leaves the constant row valid, so the LayerNorm of a row without variance reaches an output)."""
    i = R.inputs(384, 96)
    for k in ("xb", "o", "wo", "w1", "w2", "wq"):
        assert torch.equal(i[k].to(torch.bfloat16).float(), i[k]), k
    assert float(i["x"][R.CONST_ROW].var()) == 0.0 and float(i["o"][R.CONST_ROW].abs().max()) == 0.0
    assert abs(float(i["x"].mean()) - 1.5) < 0.01 and abs(float(i["x"].std()) - 0.4) < 0.01
    p = R.mask_pattern("prefix", 257)
    assert p[:50].all() and not p[50:100].any() and p[100:137].all() and not p[137:150].any() and p[150] and not p[151:200].any()
    assert bool(p[R.CONST_ROW])
    t = R.mask_pattern("tile", 257)
    assert t[:128].all() and not t[128:256].any() and t[256]
    assert R.mask_pattern("none", 5) is None and R.mask_pattern("ones", 5).all() and not R.mask_pattern("zeros", 5).any()
    for name in R.MASKS[1:]:
        assert torch.equal(R.mask_pattern(name, 387)[:129], R.mask_pattern(name, 129))
    assert max(R.ROWS) + 130 <= R.NROWS


def test_case_tables_are_the_issues():
    assert R.ROWS == (1, 16, 17, 32, 33, 64, 65, 127, 128, 129, 257) and R.INNER2 == (32, 64, 96, 128, 160)
    assert R.ROWS4 == (1, 31, 32, 33, 127, 128, 129) and R.INNER4 == (64, 96, 160)
    assert R.SPLIT_CASES == ((129, 64, 1), (129, 128, 2), (17, 192, 3), (129, 192, 2), (257, 1536, 24), (130, 1536, 16), (1, 128, 2))
    for key in ENTRY_KEYS:
        mine = [c for c in CASES if entry_key(c) == key]
        shapes = {(c.R, c.inner) for c in mine}
        if key.startswith("split"):
            assert {(c.R, c.inner, c.splits) for c in mine} >= set(R.SPLIT_CASES), key
            for c in mine:
                assert (c.inner // 32) % c.splits == 0 and (c.inner // 32) // c.splits >= 2, c.label
        elif key in ("ffn_fused", "ffn_prenorm"):
            for dim in (256, 384):
                have = {(c.R, c.inner) for c in mine if c.dim == dim}
                assert have >= {(r, 96) for r in R.ROWS4} | {(129, i) for i in R.INNER4}, (key, dim)
        else:
            lo = 32 if key == "ffn_prenorm2" else 64
            assert shapes >= {(r, 96) for r in R.ROWS} | {(129, i) for i in R.INNER2 if i >= lo} | {(257, 160), (129, 1536)}, key
            assert any(c.mask == "tile" and (c.R, c.inner) == (257, 160) for c in mine), key
            assert min(c.inner for c in mine) == lo, key
        # flags and masks: every pattern, with every flag set the entry permits
        flag_sets = {"split": (0,), "split_proj": (0, R.MASK_ACC)}.get(key, R.FLAG_SETS)
        for m in R.MASKS[1:]:
            for fl in flag_sets:
                assert any(c.mask == m and c.flags == fl for c in mine), (key, m, fl)
        assert any(c.mask == "none" and c.flags == 0 for c in mine), key
    assert sum(c.inner == 1536 for c in CASES) <= 3 * len(ENTRY_KEYS)


def test_rounding_figures_are_under_the_old_ceilings_and_above_zero():
    """e_round per case and output: <= 0.06 max / 6e-3 rms (tests/test_gpu_kernels.py), > 0 unless no row is kept; and the q/kv
    product's own rounding <= 0.08.  The `rounded` evaluation itself passes its bound (a third / two thirds of it at >= 128 rows)."""
    worst = {}
    for c in CASES:
        exact, e = R.reference(c)
        mask = R.mask_pattern(c.mask, R.bound_rows(c))
        for k, v in e.items():
            for mx, rms in (v if k == "parts" else [v]):
                assert mx <= R.CEIL_MAX and rms <= R.CEIL_RMS, f"{c.label} {k}: e_round {mx:.3e} / {rms:.3e}"
                # no row kept: MASK_OUT, the combine pass's y, and MASK_ACC where the residual is the (exact) input row
                flags_zero = c.flags & R.MASK_OUT or (c.flags & R.MASK_ACC and c.entry not in R.PROJ_ENTRIES)
                all_masked = mask is not None and not bool(mask.any()) and (flags_zero or k == "y")
                assert (mx == 0.0) == bool(all_masked) and (rms == 0.0) == bool(all_masked), f"{c.label} {k}: e_round {mx:.3e} / {rms:.3e}"
                w = worst.setdefault(entry_key(c), [0.0, 0.0])
                w[0], w[1] = max(w[0], mx), max(w[1], rms)
        rnd = R.evaluate(c, rounded=True)
        r = R.ratios(c, rnd)
        assert R.masked_rows_are_zero(c, rnd), c.label
        lim = 1.0 if c.R < 128 else 1.0 / R.RMS_FACTOR + 1e-9
        assert max(r.values()) <= lim, f"{c.label}: the rounded evaluation against its own bound {r}"
        if c.has("qkv"):
            i = R.inputs(c.dim, c.inner)
            own = rnd["out"]
            d = (R.qkv_ref(own, i["fg"], i["fb"], i["wq"], rounded=True) - R.qkv_ref(own, i["fg"], i["fb"], i["wq"])).abs()
            assert 0.0 < float(d.max()) <= R.CEIL_QKV, c.label
    print("\nworst e_round per entry (max, rms) against the ceilings 0.06 / 6e-3")
    for k, (mx, rms) in sorted(worst.items()):
        print(f"  {k:24s} {mx:.3e} {rms:.3e}")


# ------------------------------------------------------------------------------------------------ mutants


def _killed(c, mutant):
    """The worst ratio of the mutant's outputs at case c to the bound (inf for a bit-level kill); > 1 kills."""
    if mutant == "combine_reverse_order":        # bit-level only: the fp32 sums of the (fp32) parts in the other order
        rnd = R.evaluate(c, rounded=True)
        x = None if c.entry == "split_proj" else R.inputs(c.dim, c.inner)["x"][:c.R].numpy()
        parts = rnd["parts"].float().numpy()
        mask = R.mask_pattern(c.mask, c.R)
        a, b = R.combine_f32(x, parts, mask), R.combine_f32(x, parts, mask, reverse=True)
        return float("inf") if a.tobytes() != b.tobytes() else 0.0
    got = R.evaluate(c, rounded=True, mutant=mutant)
    worst = max(R.ratios(c, got).values())
    return float("inf") if not R.masked_rows_are_zero(c, got) else worst


def test_every_mutant_is_killed_for_every_entry():
    table, survivors = {}, []
    for m in R.MUTANTS:
        for key in ENTRY_KEYS:
            mine = [c for c in CASES if entry_key(c) == key and R.applies(m, c)]
            if not mine:
                continue
            for c in mine:
                ratio = _killed(c, m)
                if ratio > 1.0:
                    table[(m, key)] = (c, ratio)
                    break
            else:
                survivors.append((m, key))
    print("\nmutant x entry -> first killing case, worst figure / bound")
    for (m, key), (c, ratio) in table.items():
        print(f"  {m:24s} {key:24s} {c.label:90s} {ratio:.3g}")
    assert not survivors, survivors
    assert {m for m, _ in table} == set(R.MUTANTS)
    # the smallest kills are still clear of the bound: no mutant hides within a factor 2 of it
    assert min(r for _, r in table.values()) >= 2.0


@pytest.mark.parametrize("mutant", ["drop_first_chunk", "drop_last_chunk", "k_half_tail"])
def test_a_lost_chunk_shows_at_the_production_inner(mutant):
    """One chunk of 48 (or the second K-half of 8 of its hidden units) at inner 1536, where a chunk's share of the sum is smallest."""
    n = 0
    for c in CASES:
        if c.inner == 1536:
            assert _killed(c, mutant) > 1.0, c.label
            n += 1
    assert n >= len(ENTRY_KEYS)


# ------------------------------------------------------------------------------------------------ the four-wave kernel's instances

# ffn_bf16_kernel<KC, B1, PK, EP, ST = false, LN, LX> as ffn_launch instantiates it (csrc/ffn.hip, ISPK_FFN_KC), per KC
INSTANCES = [
    (False, True, "hot", True, True), (False, True, "dyn", True, True), (False, True, "hot", False, True), (False, True, "dyn", False, True),
    (False, True, "hot", False, False), (False, True, "dyn", False, False), (False, False, "dyn", False, False),
    (True, True, "dyn", False, False), (True, False, "dyn", False, False),
]


def test_dispatch_restatement_and_instance_coverage():
    want = {(kc,) + inst for kc in (4, 6) for inst in INSTANCES}
    assert len(want) == 18
    every = set()
    for dim in (256, 384):
        for bias1 in (False, True):
            for packed in (False, True):
                for flags in R.FLAG_SETS:
                    for bias2 in (False, True):
                        for resid in (False, True):
                            every.add(R.ffn4_instance(dim, bias1, packed, flags, bias2, resid, False, False))
        for flags in R.FLAG_SETS:
            for bias2 in (False, True):
                for stats in (False, True):
                    every.add(R.ffn4_instance(dim, False, True, flags, bias2, True, True, stats))
    assert every == want
    reached = {R.case_instance(c) for c in CASES if c.entry in ("ffn_fused", "ffn_prenorm")}
    assert reached == want, sorted(want - reached)
    # ... and every instance at every shape of the four-wave table
    for dim in (256, 384):
        for shape in R.shapes4():
            have = {R.case_instance(c) for c in R.cases4() if c.dim == dim and (c.R, c.inner) == shape}
            assert len(have) == 9, (dim, shape)


# ------------------------------------------------------------------------------------------------ argument checks

E_NULL, E_SHAPE, E_ALIGN, E_UNSUP = -1, -2, -3, -4
P, P8, P4 = ctypes.c_void_p(16), ctypes.c_void_p(8), ctypes.c_void_p(4)

# entry point -> a valid call in the order of the C signature (rows == 0 where the entry has rows)
VALID = {
    "ispk_ffn_bf16": dict(x=P, ldx=384, W1=P, ldw1=384, bias1=None, W2=P, ldw2=1536, bias2=P, resid=P, ldr=384, mask=None, out=P, ldo=384,
                          rows=0, dim=384, inner=1536, flags=0, stream=None),
    "ispk_ffn_bf16_prenorm": dict(x=P, ldx=384, gamma=P, beta=P, eps=1e-5, W1=P, ldw1=384, W2p=P, bias2=None, mask=None, out=P, ldo=384,
                                  rows=0, dim=384, inner=1536, flags=0, row_stats=None, stats_eps=1e-5, stream=None),
    "ispk_ffn_pack_w2_bf16": dict(W2=P, ldw2=1536, dim=384, inner=1536, packed=P, stream=None),
    "ispk_ffn_chunk_w2_bf16": dict(W2=P, ldw2=1536, dim=384, inner=1536, out=P, stream=None),
    "ispk_chunk_k16_bf16": dict(W=P, ldw=384, N=512, K=384, out=P, stream=None),
    "ispk_ffn_combine_ln_f32": dict(x=P, ldx=384, parts=P, part_stride=128 * 384, splits=4, mask=None, y=P, ldy=384, ln_gamma=P, ln_beta=P,
                                    ln_eps=1e-5, ln_mask=0, ln_out=P, ld_ln=384, ln_bf16=0, rows=0, dim=384, stream=None),
}
LAUNCHES = ("ispk_ffn_pack_w2_bf16", "ispk_ffn_chunk_w2_bf16", "ispk_chunk_k16_bf16")     # no row count: a valid call launches
# entry point -> [(change, expected code, the name its message carries)]
REFUSALS = {
    "ispk_ffn_bf16": [
        (dict(), 0, None), (dict(dim=256, ldx=256, ldw1=256, ldo=256, ldr=256), 0, None), (dict(ldw2=0), 0, None), (dict(inner=64), 0, None),
        (dict(x=None), E_NULL, b"ffn:"), (dict(W2=None), E_NULL, b"ffn:"), (dict(out=None), E_NULL, b"ffn:"),
        (dict(dim=128), E_UNSUP, b"ffn:"), (dict(rows=-1), E_SHAPE, b"ffn:"), (dict(inner=32), E_SHAPE, b"ffn:"),
        (dict(inner=80), E_SHAPE, b"ffn:"), (dict(flags=R.GELU), E_UNSUP, b"ffn:"), (dict(flags=R.MASK_OUT), E_NULL, b"ffn:"),
        (dict(flags=R.MASK_ACC), E_NULL, b"ffn:"), (dict(ldx=380), E_ALIGN, b"ffn:"), (dict(ldx=376), E_ALIGN, b"ffn:"),
        (dict(ldw1=388), E_ALIGN, b"ffn:"), (dict(ldw2=1528), E_ALIGN, b"ffn:"), (dict(ldw2=1540), E_ALIGN, b"ffn:"),
        (dict(ldo=386), E_ALIGN, b"ffn:"), (dict(ldo=380), E_ALIGN, b"ffn:"), (dict(ldr=386), E_ALIGN, b"ffn:"),
        (dict(x=P8), E_ALIGN, b"ffn:"), (dict(resid=P8), E_ALIGN, b"ffn:"), (dict(bias2=P8), E_ALIGN, b"ffn:"), (dict(out=P8), E_ALIGN, b"ffn:")],
    "ispk_ffn_bf16_prenorm": [
        (dict(), 0, None), (dict(dim=256, ldx=256, ldw1=256, ldo=256), 0, None), (dict(ldx=388), 0, None),
        (dict(x=None), E_ALIGN, b"ffn_prenorm:"), (dict(x=P8), E_ALIGN, b"ffn_prenorm:"), (dict(W1=None), E_NULL, b"ffn:"),
        (dict(W2p=None), E_NULL, b"ffn:"), (dict(dim=512), E_UNSUP, b"ffn:"), (dict(inner=32), E_SHAPE, b"ffn:"),
        (dict(flags=R.GELU), E_UNSUP, b"ffn:"), (dict(flags=R.MASK_OUT), E_NULL, b"ffn:"), (dict(ldx=386), E_ALIGN, b"ffn:"),
        (dict(ldx=380), E_ALIGN, b"ffn:"), (dict(ldo=380), E_ALIGN, b"ffn:"), (dict(bias2=P8), E_ALIGN, b"ffn:")],
    "ispk_ffn_pack_w2_bf16": [
        (dict(W2=None), E_NULL, b"ffn_pack_w2:"), (dict(packed=None), E_NULL, b"ffn_pack_w2:"), (dict(dim=0), E_SHAPE, b"ffn_pack_w2:"),
        (dict(inner=0), E_SHAPE, b"ffn_pack_w2:"), (dict(inner=48, ldw2=48), E_SHAPE, b"ffn_pack_w2:"), (dict(ldw2=1528), E_SHAPE, b"ffn_pack_w2:")],
    "ispk_ffn_chunk_w2_bf16": [
        (dict(W2=None), E_NULL, b"ffn_chunk_w2:"), (dict(out=None), E_NULL, b"ffn_chunk_w2:"), (dict(dim=0), E_SHAPE, b"ffn_chunk_w2:"),
        (dict(inner=16, ldw2=16), E_SHAPE, b"ffn_chunk_w2:"), (dict(inner=48, ldw2=48), E_SHAPE, b"ffn_chunk_w2:"),
        (dict(ldw2=1528), E_SHAPE, b"ffn_chunk_w2:"), (dict(ldw2=1540), E_ALIGN, b"ffn_chunk_w2:"), (dict(W2=P8), E_ALIGN, b"ffn_chunk_w2:"),
        (dict(out=P8), E_ALIGN, b"ffn_chunk_w2:")],
    "ispk_chunk_k16_bf16": [
        (dict(W=None), E_NULL, b"chunk_k16:"), (dict(out=None), E_NULL, b"chunk_k16:"), (dict(N=0), E_SHAPE, b"chunk_k16:"),
        (dict(K=8, ldw=8), E_SHAPE, b"chunk_k16:"), (dict(K=24, ldw=24), E_SHAPE, b"chunk_k16:"), (dict(ldw=376), E_SHAPE, b"chunk_k16:"),
        (dict(ldw=388), E_ALIGN, b"chunk_k16:"), (dict(W=P8), E_ALIGN, b"chunk_k16:"), (dict(out=P8), E_ALIGN, b"chunk_k16:")],
    "ispk_ffn_combine_ln_f32": [
        (dict(), 0, None), (dict(x=None, ldx=0), 0, None), (dict(ln_out=None, ln_gamma=None, ln_beta=None), 0, None), (dict(splits=1), 0, None),
        (dict(ln_out=P8, ln_bf16=1), 0, None), (dict(part_stride=0), 0, None),
        (dict(parts=None), E_NULL, b"ffn_combine_ln:"), (dict(y=None), E_NULL, b"ffn_combine_ln:"), (dict(dim=256), E_SHAPE, b"ffn_combine_ln:"),
        (dict(rows=-1), E_SHAPE, b"ffn_combine_ln:"), (dict(splits=0), E_SHAPE, b"ffn_combine_ln:"), (dict(ldx=380), E_SHAPE, b"ffn_combine_ln:"),
        (dict(ldx=386), E_SHAPE, b"ffn_combine_ln:"), (dict(ldy=380), E_SHAPE, b"ffn_combine_ln:"), (dict(ldy=386), E_SHAPE, b"ffn_combine_ln:"),
        (dict(part_stride=386), E_SHAPE, b"ffn_combine_ln:"), (dict(ln_gamma=None), E_NULL, b"ffn_combine_ln:"),
        (dict(ln_beta=None), E_NULL, b"ffn_combine_ln:"), (dict(ld_ln=380), E_NULL, b"ffn_combine_ln:"), (dict(ld_ln=386), E_NULL, b"ffn_combine_ln:"),
        (dict(x=P8), E_ALIGN, b"ffn_combine_ln:"), (dict(parts=P8), E_ALIGN, b"ffn_combine_ln:"), (dict(y=P8), E_ALIGN, b"ffn_combine_ln:"),
        (dict(ln_out=P4), E_ALIGN, b"ffn_combine_ln:")],
}


@pytest.mark.parametrize("entry", sorted(VALID))
def test_argument_checks(entry):
    lib = runtime.lib()
    valid = VALID[entry]
    for change, want, name in REFUSALS[entry]:
        assert set(change) <= set(valid), change
        assert want != 0 or entry not in LAUNCHES
        got = getattr(lib, entry)(*{**valid, **change}.values())
        assert got == want, f"{entry}{change}: {got}, expected {want} ({lib.ispk_last_error_string()!r})"
        if want != 0:
            assert name in lib.ispk_last_error_string(), f"{entry}{change}: {lib.ispk_last_error_string()!r}"
