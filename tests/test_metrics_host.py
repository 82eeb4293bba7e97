"""CPU: the evaluator's host side - the restated DCT-II basis (torchaudio.functional.create_dct), the argument checks of
ispk_acoustic_metrics_f32 (they run before any launch), and the evaluator fixture's inputs against synth's keyed streams."""
import ctypes
import math

import numpy as np
import pytest
import torch

from conftest import crc, golden

from isp_tts_amd import runtime, synth
from isp_tts_amd.acoustic import create_dct


def test_create_dct_matches_scipy():
    fft = pytest.importorskip("scipy.fft")
    for n_mfcc, n_mels in ((13, 80), (20, 80), (80, 80), (1, 7)):
        d = create_dct(n_mfcc, n_mels, norm="ortho")
        assert d.shape == (n_mels, n_mfcc) and d.dtype == torch.float32
        ref = fft.dct(np.eye(n_mels), norm="ortho")[:, :n_mfcc]       # row n: the DCT-II of e_n
        assert np.abs(d.double().numpy() - ref).max() < 1e-7
    ref = fft.dct(np.eye(80))[:, :13]                                 # norm=None: the unscaled 2 cos(...) sums
    assert np.abs(create_dct(13, 80, norm=None).double().numpy() - ref).max() < 1e-5


def test_create_dct_is_orthonormal():
    d = create_dct(80, 80).double()
    assert torch.allclose(d.T @ d, torch.eye(80, dtype=torch.float64), atol=1e-6)
    d13 = create_dct(13, 80).double()
    assert torch.allclose(d13.T @ d13, torch.eye(13, dtype=torch.float64), atol=1e-6)
    assert abs(float(d13[0, 0]) - 1 / math.sqrt(80)) < 1e-7
    with pytest.raises(ValueError):
        create_dct(13, 80, norm="slaney")


def test_metrics_argument_errors_without_gpu():
    lib = runtime.lib()
    one = ctypes.c_void_p(16)  # never dereferenced: argument checks fail first

    def rc(mo=one, mt=one, ml=one, tl=one, at=one, dct=one, ws=one, wn=1 << 20, out=one, B=2, C=80, T=40, L=10, n=13):
        return lib.ispk_acoustic_metrics_f32(mo, 3200, 40, 1, mt, 3200, 40, 1, ml, tl, at, 400, 10, dct, ws, wn, out, B, C, T, L,
                                             n, None)

    assert rc(ml=None) == -1 and b"null" in lib.ispk_last_error_string()
    assert rc(out=None) == -1 and rc(ws=None) == -1
    assert rc(mo=None) == -1 and rc(mt=None) == -1 and rc(dct=None) == -1
    assert rc(mo=None, mt=None, at=None) == -1
    assert rc(tl=None) == -1
    assert rc(B=0) == -2 and rc(B=65536) == -2 and rc(T=0) == -2 and rc(L=0) == -2
    assert rc(C=129) == -2 and b"128" in lib.ispk_last_error_string()
    assert rc(C=0) == -2 and rc(n=0) == -2 and rc(n=81) == -2
    assert rc(wn=3 * 2 * 2 - 1) == -3 and b"12 floats" in lib.ispk_last_error_string()
    # a half without its operands is not checked: mels absent -> no DCT / C / n_mfcc needed; attention absent -> no L / text_len
    assert rc(mo=None, mt=None, dct=None, C=0, n=0, B=0) == -2           # (still refused: B = 0)
    assert rc(at=None, tl=None, L=0, B=0) == -2
    assert runtime.metrics_workspace_floats(64, 512) == 3 * 64 * 16 and runtime.metrics_workspace_floats(5, 65) == 45


def test_metrics_wrapper_needs_gpu_tensors():
    with pytest.raises(runtime.IspkError, match="GPU tensors"):
        runtime.acoustic_metrics(torch.zeros(1, 80, 4), torch.zeros(1, 80, 4), torch.tensor([4]), torch.tensor([2]),
                                 torch.zeros(1, 4, 3), create_dct(13, 80))


def test_mel_layout_rule_is_the_references():
    """MCD._mfcc (evaluator.py:28-31) transposes unless size(-1) == n_mel_channels: [B, C, T] and [B, T, C] read frames
    along T, and a [B, 80, 80] mel is read frames-first (its axes swapped relative to the collator's layout)."""
    x = torch.zeros(2, 80, 50)
    assert runtime._mel_strides(x, 80) == (80, 50, 4000, 50, 1)
    assert runtime._mel_strides(x.transpose(1, 2).contiguous(), 80) == (80, 50, 4000, 1, 80)
    q = torch.zeros(2, 80, 80)
    assert runtime._mel_strides(q, 80) == (80, 80, 6400, 1, 80)


def test_fixture_inputs_come_from_synth():
    g = golden("metrics.npz")
    for case in synth.METRIC_CASES:
        d = synth.make_metric_inputs(case)
        assert [crc(d[k]) for k in ("mel_out", "mel_target", "attn_soft", "mel_len", "text_len")] == \
            [int(v) for v in g[f"{case}_crc"]], case
        B, T, L = d["attn_soft"].shape
        assert int(d["mel_len"].max()) == T and int(d["mel_len"].min()) >= 1
        assert g[f"{case}_values"].shape == (3,) and np.isfinite(g[f"{case}_values"]).all()
    assert g["forward_values"].shape == (3,) and g["forward_crc"].shape == (6,)
    assert g["t80_crc"].shape == (5,) and synth.make_metric_inputs("t80")["mel_out"].shape == (2, 80, 80)
