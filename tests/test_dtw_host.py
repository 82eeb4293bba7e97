"""CPU: the host side of the DTW scorer - the two entry points in the header and in runtime.SIGNATURES, their argument checks
(they run before any launch), the workspace sizes, and the float64 reference (tests/dtw_reference.py) against cases solved by
hand."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

import dtw_reference as ref
from isp_tts_amd import runtime
from isp_tts_amd.acoustic import SynthesisEvaluator, create_dct

E_NULL, E_SHAPE, E_WORKSPACE = -1, -2, -3


def test_header_and_signatures_list_both_entries():
    src = open(os.path.join(ROOT, "include", "ispk.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, nargs in (("ispk_dtw_f32", 14), ("ispk_mcd_dtw_f32", 26)):
        m = re.search(r"int32_t\s+" + name + r"\s*\(([^)]*)\)", src)
        assert m, f"{name} is not declared in include/ispk.h"
        assert len(m.group(1).split(",")) == nargs == len(runtime.SIGNATURES[name])
        assert hasattr(runtime.lib(), name)
    assert runtime.lib().ispk_abi_version() == 2


def _dtw_rc(cost=16, nl=16, ml=16, total=16, steps=16, path=None, ws=16, wn=1 << 30, B=2, N=40, M=50):
    p = lambda v: ctypes.c_void_p(v) if v else None   # noqa: E731  (never dereferenced: the argument checks fail first)
    lib = runtime.lib()
    return lib.ispk_dtw_f32(p(cost), N * M, M, p(nl), p(ml), p(total), p(steps), p(path), p(ws), wn, B, N, M, None), \
        lib.ispk_last_error_string()


def test_dtw_argument_errors_without_gpu():
    for k in ("cost", "nl", "ml", "total", "steps", "ws"):
        rc, msg = _dtw_rc(**{k: None})
        assert rc == E_NULL and b"null" in msg, k
    for kw in (dict(N=0), dict(M=0), dict(N=2049), dict(M=2049), dict(B=-1), dict(B=65536)):
        assert _dtw_rc(**kw)[0] == E_SHAPE, kw
    assert b"2048" in _dtw_rc(N=2049)[1]
    need = runtime.dtw_workspace_floats(2, 40, 50)
    assert need == 2 * 256 * (305 + 4)           # R = 1: 50 + 255 rows of the skewed costs, ceil(50 / 16) back-pointer words per lane
    rc, msg = _dtw_rc(wn=need - 1)
    assert rc == E_WORKSPACE and str(need).encode() in msg
    assert _dtw_rc(ws=20)[0] == E_WORKSPACE and b"aligned" in _dtw_rc(ws=20)[1]
    assert _dtw_rc(B=0)[0] == 0                                      # a no-op, before any launch
    assert _dtw_rc(B=0, N=2049)[0] == E_SHAPE                        # (the shape is still checked)


def _mcd_rc(mo=16, mt=16, dct=16, nl=16, ml=16, po=None, pt=None, ws=16, wn=1 << 40, items=16, means=16, cost=None, B=2, C=80,
            N=40, M=50, n=13):
    p = lambda v: ctypes.c_void_p(v) if v else None   # noqa: E731
    lib = runtime.lib()
    return lib.ispk_mcd_dtw_f32(p(mo), C * N, N, 1, p(mt), C * M, M, 1, p(dct), p(nl), p(ml), p(po), N, p(pt), M, p(ws), wn,
                                p(items), p(means), p(cost), B, C, N, M, n, None), lib.ispk_last_error_string()


def test_mcd_dtw_argument_errors_without_gpu():
    for k in ("mo", "mt", "dct", "nl", "ml", "ws", "items", "means"):
        rc, msg = _mcd_rc(**{k: None})
        assert rc == E_NULL and b"null" in msg, k
    assert _mcd_rc(po=16)[0] == E_NULL and _mcd_rc(pt=16)[0] == E_NULL      # one pitch track without the other
    for kw in (dict(N=0), dict(M=0), dict(N=2049), dict(M=2049), dict(B=-1), dict(B=65536), dict(C=0), dict(C=129), dict(n=0),
               dict(n=81)):
        assert _mcd_rc(**kw)[0] == E_SHAPE, kw
    assert b"128" in _mcd_rc(C=129)[1]
    need = runtime.mcd_dtw_workspace_floats(2, 40, 50, 13)
    assert need == 2 * 256 * (305 + 4) + 2 * 90 * 12 + 4
    rc, msg = _mcd_rc(wn=need - 1)
    assert rc == E_WORKSPACE and str(need).encode() in msg
    assert _mcd_rc(ws=24)[0] == E_WORKSPACE and b"aligned" in _mcd_rc(ws=24)[1]
    assert _mcd_rc(B=0)[0] == 0 and _mcd_rc(B=0, po=16, pt=16, cost=16)[0] == 0


def test_workspace_sizes_follow_the_rows_per_lane():
    # at the limit: 2,303 rows of 2,048 skewed costs, and 2 bits per cell (1 MiB) of back-pointers
    assert runtime.dtw_workspace_floats(1, 2048, 2048) == 2303 * 2048 + 2048 * 2048 // 16
    assert runtime.dtw_workspace_floats(3, 256, 17) == 3 * 256 * (272 + 2)          # R = 1
    assert runtime.dtw_workspace_floats(1, 257, 17) == 256 * (272 * 2 + 3)          # R = 2: 8 columns per word
    assert runtime.dtw_workspace_floats(1, 513, 17) == 256 * (272 * 4 + 5)          # R = 4
    assert runtime.dtw_workspace_floats(1, 1025, 17) == 256 * (272 * 8 + 9)         # R = 8


def test_wrappers_need_gpu_tensors():
    with pytest.raises(runtime.IspkError, match="GPU tensors"):
        runtime.dtw(torch.zeros(1, 4, 4), torch.tensor([4]), torch.tensor([4]))
    with pytest.raises(runtime.IspkError, match="GPU tensors"):
        runtime.mcd_dtw(torch.zeros(1, 80, 4), torch.tensor([4]), torch.zeros(1, 80, 5), torch.tensor([5]), create_dct(13, 80))
    with pytest.raises(ValueError, match="both pitch tracks"):
        SynthesisEvaluator()(torch.zeros(1, 80, 4), torch.tensor([4]), torch.zeros(1, 80, 5), torch.tensor([5]),
                             pitch_out=torch.zeros(1, 4))


# ---------------------------------------------------------------------------------------------------- the reference, by hand
HAND = [
    # cost, total, path
    ([[7.0]], 7.0, [(0, 0)]),
    ([[1, 2], [3, 4]], 5.0, [(0, 0), (1, 1)]),
    # D = [[0, 0], [0, 1]]: all three predecessors of (1, 1) hold 0 -> the diagonal (K = 2, not 3)
    ([[0, 0], [0, 1]], 1.0, [(0, 0), (1, 1)]),
    # D = [[5, 4], [4, .]]: (i-1, j) and (i, j-1) tie below the diagonal -> (i-1, j) = (0, 1)
    ([[5, -1], [-1, 2]], 6.0, [(0, 0), (0, 1), (1, 1)]),
    # a row and a column have one path
    ([[1, 2, 3, 4]], 10.0, [(0, 0), (0, 1), (0, 2), (0, 3)]),
    ([[1], [2], [3]], 6.0, [(0, 0), (1, 0), (2, 0)]),
    # D = [[1, 4, 9], [5, 2, 4], [11, 4, 3]]
    ([[1, 3, 5], [4, 1, 2], [6, 2, 1]], 3.0, [(0, 0), (1, 1), (2, 2)]),
    # D = [[1, 2, 3], [10, 10, 3]]: along the cheap row, then the diagonal into the corner
    ([[1, 1, 1], [9, 9, 1]], 3.0, [(0, 0), (0, 1), (1, 2)]),
    # D = [[2, 4], [3, 4], [4, 5]]: (1, 1) takes the diagonal (2 < 3 < 4); the corner's diagonal (3) beats up (4) and left (4)
    ([[2, 2], [1, 2], [1, 2]], 5.0, [(0, 0), (1, 0), (2, 1)]),
]


@pytest.mark.parametrize("k", range(len(HAND)))
def test_reference_against_hand_solved_cases(k):
    cost, total, path = HAND[k]
    for fn in (ref.dtw, ref.dtw_cellwise):
        t, p = fn(np.array(cost, dtype=np.float64))
        assert t == total and [tuple(v) for v in p] == path, fn.__name__
        assert ref.is_warping_path(p, len(cost), len(cost[0])) and ref.path_cost(cost, p) == total


def test_reference_diagonal_fill_equals_the_cellwise_one():
    g = np.random.default_rng(5)
    for n, m, hi in ((1, 9, 3), (9, 1, 3), (17, 23, 2), (40, 31, 4), (33, 33, 1), (64, 65, 3)):
        c = g.integers(0, hi, size=(n, m)).astype(np.float64)        # small integers: ties everywhere
        t0, p0 = ref.dtw_cellwise(c)
        t1, p1 = ref.dtw(c)
        assert t0 == t1 and np.array_equal(p0, p1)
        assert ref.is_warping_path(p1, n, m) and max(n, m) <= len(p1) <= n + m - 1
    pad = ref.padded_path(p1, 70, 70)
    assert pad.dtype == np.int16 and pad.shape == (139, 2) and (pad[len(p1):] == -1).all() and np.array_equal(pad[:len(p1)], p1)


def test_reference_scores_by_hand():
    path = [(0, 0), (1, 1), (1, 2), (2, 3)]
    f_out = np.array([100.0, 0.0, 200.0])
    f_tgt = np.array([200.0, 0.0, 50.0, 100.0])
    # pairs: (100, 200) both voiced: -1200 cents; (0, 0) both unvoiced; (0, 50) differ; (200, 100) both voiced: +1200 cents
    s = ref.scores(8.0, path, 3, 4, f_out, f_tgt)
    assert s["mcd_dtw"] == ref.LOGDB * 2.0 and s["length_ratio"] == 0.75
    assert abs(s["f0_rmse_cents"] - 1200.0) < 1e-9 and s["vuv_error"] == 0.25
    s = ref.scores(8.0, path, 3, 4, np.zeros(3), f_tgt)
    assert np.isnan(s["f0_rmse_cents"]) and s["vuv_error"] == 0.75
    assert set(ref.scores(1.0, path, 3, 4)) == {"mcd_dtw", "length_ratio"}
    assert not ref.is_warping_path([(0, 0), (2, 1)], 3, 2) and not ref.is_warping_path([(0, 1), (1, 1)], 2, 2)
    assert not ref.is_warping_path([(0, 0), (1, 1)], 3, 2)


def test_reference_cepstral_cost_drops_coefficient_0():
    g = np.random.default_rng(1)
    a, b = g.standard_normal((80, 5)), g.standard_normal((80, 7))
    dct = create_dct(13, 80).double().numpy()
    c = ref.cepstral_cost(a, b, dct)
    assert c.shape == (5, 7)
    assert np.allclose(ref.cepstral_cost(a + 3.0, b - 2.0, dct), c, atol=1e-6)       # a level shift lives in coefficient 0 only
    assert abs(c[2, 3] - np.linalg.norm((a[:, 2] - b[:, 3]) @ dct[:, 1:])) < 1e-12
