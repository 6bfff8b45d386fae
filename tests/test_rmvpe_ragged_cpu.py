"""Host-side parts of the ragged RMVPE path: the per-row sizes ``RMVPE.get_pitch_batch`` works out before anything
is launched, against the restatements the GPU tests use, and the library table's three ragged entries."""
import os
import re

import numpy as np
import pytest

from prodiff_amd import _lib
from prodiff_amd import rmvpe as RM
from tests import rmvpe_cases as RC
from tests import rmvpe_ref as R
from tests import viterbi_ref as V
from tests.test_cpu_host import ROOT

HEADER = os.path.join(ROOT, "include", "prodiff_hip.h")

SECONDS = (0.5, 0.31, 0.2)        # the clips of tests/test_gpu_rmvpe_ragged.py


def test_row_sizes_match_the_restatements():
    lens = [len(RC.harmonic_signal(44100, s)) for s in SECONDS]
    lens16, frames, T = RM.pitch_row_sizes(lens, 44100)
    assert lens16 == [-(-n * 160 // 441) for n in lens]                      # ceil(n L / o), as test_f0_from_audio states it
    basis = np.ones((4, 513))
    for b, n16 in enumerate(lens16):
        spec = R.centered_mel(np.zeros((1, n16)), basis)[0]                  # [1, T_b, 513]
        assert frames[b] == spec.shape[1] == 1 + n16 // 160
    assert T % 32 == 0 and T - 32 < max(frames) <= T
    t_dst = 512 / 44100
    lengths = [int(round(n / 512)) + 2 for n in lens]
    rows = RM.align_rows(frames, lengths, 0.01, t_dst)
    for (n, m, ln), f, want in zip(rows, frames, lengths):
        assert (n, ln) == (f, want)
        assert m == len(np.arange(0, (n - 1) * 0.01, t_dst))
        ref, _ = V.align_f0(np.full(n, 220.0, np.float32), 0.01, t_dst, ln)
        assert len(ref) == ln
    assert RM.align_rows(frames, 7, 0.01, t_dst) == [(n, m, 7) for n, m, _ in rows]
    # 16 kHz input is not resampled
    assert RM.pitch_row_sizes([8000, 513], 16000)[:2] == ([8000, 513], [51, 4])


def test_a_short_row_is_refused_and_named():
    assert RM.MIN_SAMPLES_16K == 513
    RM.pitch_row_sizes([513], 16000)
    with pytest.raises(ValueError, match="row 2"):
        RM.pitch_row_sizes([22050, 8820, 400], 44100)
    with pytest.raises(ValueError, match="row 0"):
        RM.pitch_row_sizes([512], 16000)
    with pytest.raises(ValueError, match="row 1"):
        RM.align_rows([51, 1], 10, 0.01, 512 / 44100)
    with pytest.raises(ValueError, match="row 0"):
        RM.align_rows([51, 21], [0, 4], 0.01, 512 / 44100)


def test_the_table_holds_the_ragged_entries():
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    for name in ("pd_rmvpe_forward_ragged", "pd_rmvpe_viterbi_ragged", "pd_f0_align_ragged"):
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, name
        res, args = _lib._SIGS[name]
        assert res is _lib.C.c_int
        assert len(args) == len(m.group(1).split(",")), name
        assert hasattr(_lib.lib(), name)
    # one more argument than the equal-length entries: the per-row lengths
    assert len(_lib._SIGS["pd_rmvpe_forward_ragged"][1]) == len(_lib._SIGS["pd_rmvpe_forward"][1]) + 1
    assert len(_lib._SIGS["pd_rmvpe_viterbi_ragged"][1]) == len(_lib._SIGS["pd_rmvpe_viterbi"][1]) + 1
