"""Host-side parts of the ragged harmonic-noise separation and variance curves: the per-row sizes worked out before
anything is launched, against the numpy / torch restatements the GPU tests use, the list stacking, and the library
table's ragged entries."""
import os
import re

import numpy as np
import pytest
import torch

from prodiff_amd import _lib
from prodiff_amd import curves as CV
from prodiff_amd import rmvpe as RM
from prodiff_amd import vr as VR
from tests import curves_cases as CC
from tests import curves_ref as CR
from tests import vr_ref as R
from tests.test_cpu_host import ROOT

HEADER = os.path.join(ROOT, "include", "prodiff_hip.h")

VR_LENS = (645, 1297, 2249, 995, 7)              # the clips of tests/test_gpu_vr_ragged.py (n_fft 128, hop 32)
CURVE_LENS = (64 * 37 + 13, 64 * 20 + 1, 64 * 9 + 5, 129)      # those of tests/test_gpu_curves_ragged.py (win 256, hop 64)


def test_vr_row_sizes_match_the_restatement():
    n_fft, hop = 128, 32
    sizes = VR.row_sizes(VR_LENS, n_fft, hop)
    assert [t for t, _ in sizes] == [32, 64, 96, 64, 32]
    for n, (T, lead) in zip(VR_LENS, sizes):
        spec, Tl_pad = R.stft(np.zeros((1, 1, n), np.float32), n_fft, hop)       # torch.stft of the padded row
        assert spec.shape[-1] == T and lead == n_fft // 2 + Tl_pad
        assert T % 32 == 0 and T - 32 <= n // hop + 1 < T
        # the kept samples lie inside the inverse transform's output, as pd_vr_istft demands
        assert lead - n_fft // 2 + n <= (T - 1) * hop
    # a frame count that is already a multiple of 32 gains a whole block
    assert VR.row_sizes([32 * 31], n_fft, hop)[0][0] == 64 and VR.row_sizes([32 * 31 - 1], n_fft, hop)[0][0] == 32
    # the longest row decides the batch's frames: no row has more
    assert max(t for t, _ in sizes) == VR.padded_frames(max(VR_LENS), hop)[0]


def test_curve_rows_match_the_restatements():
    win, hop = 256, 64
    frames = [CC.frames_of(n, hop) for n in CURVE_LENS]
    f0_lens = [t + d for t, d in zip(frames, (-2, 3, 0, 0))]
    L, Tf = max(CURVE_LENS), max(f0_lens)
    rows = CV.curve_rows(CURVE_LENS, None, f0_lens, L, Tf, win, hop)
    assert rows == list(zip(CURVE_LENS, frames, f0_lens))
    for n, m, _ in rows:
        assert m == CV.num_frames(n, hop) == CR.rms(np.zeros(n, np.float32), win, hop).shape[-1]
    for n, tf in zip(CURVE_LENS, f0_lens):
        f = CC.padded_f0(np.full(tf, 200.0, np.float32), 0, n, hop)             # the right pad to the frame count
        assert len(f) == max(tf, CC.frames_of(n, hop))
    # mel_len: an int for every row, or one per row
    assert [r[1] for r in CV.curve_rows(CURVE_LENS, 7, f0_lens, L, Tf, win, hop)] == [7] * 4
    per_row = [CC.mel_lens(n, hop)[b % 3] for b, n in enumerate(CURVE_LENS)]
    assert [r[1] for r in CV.curve_rows(CURVE_LENS, per_row, f0_lens, L, Tf, win, hop)] == per_row
    # without lens every row is the stride; a call without f0 carries zeros
    assert CV.curve_rows(None, [3, 4], None, 500, 0, win, hop) == [(500, 3, 0), (500, 4, 0)]
    assert CV.curve_rows(None, 5, [9, 8], 500, 9, win, hop) == [(500, 5, 9), (500, 5, 8)]


def test_bad_sizes_are_refused_and_named():
    win, hop = 256, 64
    CV.curve_rows([129], None, [1], 129, 1, win, hop)
    with pytest.raises(_lib.HipError, match="row 1"):
        CV.curve_rows([300, 128], None, [5, 5], 300, 5, win, hop)               # L_b <= win / 2
    with pytest.raises(_lib.HipError, match="row 0"):
        CV.curve_rows([301, 200], None, [5, 5], 300, 5, win, hop)               # past the row stride
    with pytest.raises(_lib.HipError, match="row 1"):
        CV.curve_rows([300, 200], [4, 0], [5, 5], 300, 5, win, hop)
    with pytest.raises(_lib.HipError, match="row 0"):
        CV.curve_rows([300, 200], None, [6, 5], 300, 5, win, hop)
    with pytest.raises(_lib.HipError):
        CV.curve_rows([300, 200], [4], [5, 5], 300, 5, win, hop)                # a wrong count


def test_lists_are_stacked_by_the_one_implementation():
    assert VR.stack_waveforms is RM.stack_waveforms
    clips = [np.arange(5, dtype=np.float32), np.arange(3, dtype=np.float64), torch.arange(4)]
    as_np, t, ns = CV._stack(clips, None, "cpu")
    assert as_np and ns == [5, 3, 4] and t.dtype == torch.float32 and tuple(t.shape) == (3, 5)
    assert t[1].tolist() == [0, 1, 2, 0, 0] and t[2].tolist() == [0, 1, 2, 3, 0]
    as_np, t, ns = CV._stack(torch.zeros(2, 6), [6, 2], "cpu")
    assert not as_np and ns == [6, 2] and tuple(t.shape) == (2, 6)
    with pytest.raises(_lib.HipError):
        CV._stack(torch.zeros(2, 6), [6, 7], "cpu")
    with pytest.raises(ValueError):
        CV._stack([], None, "cpu")
    got = CV._cut(True, torch.arange(12.0).reshape(2, 6), [6, 2])
    assert [g.tolist() for g in got] == [[0, 1, 2, 3, 4, 5], [6, 7]] and CV._cut(True, None, [1]) is None


RAGGED = {   # ragged entry -> (equal-length entry, arguments more than it)
    "pd_vr_separate_ragged": ("pd_vr_separate", 1),
    "pd_vr_mask_ragged": ("pd_vr_mask", 1),
    "pd_vr_stft_ragged": ("pd_vr_stft", 0),       # lens replaces the scalar lead
    "pd_vr_istft_ragged": ("pd_vr_istft", 0),
    "pd_curves_kth_harmonic_ragged": ("pd_curves_kth_harmonic", 1),
    "pd_curves_energy_ragged": ("pd_curves_energy", 1),
    "pd_curves_forward_ragged": ("pd_curves_forward", 1),
}


def test_the_table_holds_the_ragged_entries():
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    for name, (equal, more) in RAGGED.items():
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, name
        res, args = _lib._SIGS[name]
        assert res is _lib.C.c_int
        assert len(args) == len(m.group(1).split(",")), name
        assert hasattr(_lib.lib(), name), name
        assert len(args) == len(_lib._SIGS[equal][1]) + more, name
        assert "const int*" in m.group(1) and "int*" not in re.sub(r"const int\*", "", m.group(1), count=1), name
