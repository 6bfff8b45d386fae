"""CPU tests around the native Viterbi decode and f0 tail: the reduced (band + global maximum) recurrence equals
the dense one bit for bit, the case inputs are robust (the reference's float32 normalisation and 1e-6 noise on the
log-probabilities leave every path unchanged, no interpolated unvoiced flag sits at the 0.5 threshold), the tables
the Python side hands to the kernel are the restatement's, and the public surface is in place."""
import ctypes as C

import numpy as np
import pytest
import torch

import prodiff_amd
from prodiff_amd import _lib
from prodiff_amd import rmvpe as RM
from tests import viterbi_ref as V

# (case, T, n, w): every case at the full state space, plus the small state spaces of the GPU test
CASES = [(name, T, 360, 30) for name in V.CASE_NAMES for T in (1, 2, 33, 64)] + \
        [("rand", 300, 360, 30), ("glide", 300, 360, 30), ("jump", 65, 40, 5), ("rand", 65, 40, 5), ("rand", 65, 8, 30),
         ("glide", 65, 8, 30), ("rand", 40, 100, 40)]


@pytest.mark.parametrize("name,T,n,w", CASES)
def test_banded_equals_dense(name, T, n, w):
    h = V.case(name, T, n)
    val_d, path_d = V.dense(h, w)
    val_b, path_b = V.banded(h, w)
    assert np.array_equal(val_d, val_b)
    assert np.array_equal(path_d, path_b)


def test_the_jump_case_takes_an_out_of_band_step():
    _, path = V.dense(V.case("jump", 64))
    step = np.abs(np.diff(path))
    assert step.max() >= 200 and (step >= V.WIDTH).sum() == 1
    _, path = V.dense(V.case("uniform", 33))
    assert (path == 0).all()


@pytest.mark.parametrize("name,T", [(n, T) for n in V.CASE_NAMES for T in (33, 64)] + [("rand", 300), ("glide", 300)])
def test_case_paths_are_robust(name, T):
    """Conditions on the inputs, not on the kernel: a case that fails here gets another seed."""
    h = V.case(name, T)
    lp = V.log_prob(h)
    val, path = V.dense(h)
    if name != "uniform":        # all-equal saliences tie by construction; the tie rule, not a margin, decides
        assert np.array_equal(V.dense_f32norm(h)[1], path)
        rng = np.random.default_rng(11)
        for _ in range(3):
            noisy = lp * (1.0 + 1e-6 * rng.standard_normal(lp.shape))
            assert np.array_equal(V.dense_from_lp(noisy)[1], path)
        # the final argmax: rounding moves val by about 1e-16 T |lp| ~ 1e-11, the gap must dwarf that
        top = np.sort(val[-1])
        assert top[-1] - top[-2] >= 1e-3
    else:
        assert np.array_equal(V.dense_f32norm(h)[1], path)


def test_tables_are_the_restatements():
    for n, w in ((360, 30), (40, 5), (8, 30), (100, 40)):
        band, log_off, log_init = RM.viterbi_tables(n, w)
        lt = np.log(V.transition(n, w) + V.TINY)
        assert band.dtype == np.float64 and band.shape == (n, 2 * w - 1)
        for i in range(n):
            for j in range(max(i - w + 1, 0), min(i + w, n)):
                assert band[i, j - i + w - 1] == lt[i, j]
        off = lt[np.abs(np.arange(n)[:, None] - np.arange(n)[None, :]) >= w]
        assert (off == log_off).all() and log_off == np.log(V.TINY)
        assert log_init == np.log(1.0 / n + V.TINY)
        assert lt[lt > log_off].min() > -6.91 or w != 30


def test_resampled_length_is_numpys():
    for n in (2, 3, 17, 101, 1001, 60001):
        for t_src, t_dst in V.GRIDS + ((0.01, 0.005), (0.01, 0.02), (0.02, 0.01)):
            assert RM.resampled_length(n, t_src, t_dst) == len(np.arange(0, (n - 1) * t_src, t_dst))


def test_no_uv_value_sits_at_the_threshold():
    for n in (2, 3, 101, 1001):
        for t_src, t_dst in V.GRIDS:
            m = RM.resampled_length(n, t_src, t_dst)
            for name, row in V.f0_rows(n).items():
                u = V.uv_curve(row, t_src, t_dst, m + 2)
                assert np.abs(u - 0.5).min() > 1e-9, (n, t_dst, name)


def test_f0_tail_restatement_is_the_modules():
    """tests/viterbi_ref.py's copies agree with prodiff_amd.rmvpe's host helpers (which get_pitch runs)."""
    for n in (3, 101):
        for name, row in V.f0_rows(n).items():
            f, uv = RM.interp_f0(row.copy())
            f2, uv2 = V.interp_f0(row)
            np.testing.assert_array_equal(f, f2)
            np.testing.assert_array_equal(uv, uv2)
            for length in (5, 80, 400):
                np.testing.assert_array_equal(RM.resample_align_curve(f, 0.01, 512 / 44100, length),
                                              V.resample_align_curve(f2, 0.01, 512 / 44100, length))


def test_exports_and_surface():
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("pd_rmvpe_viterbi", "pd_rmvpe_viterbi_workspace_size", "pd_rmvpe_viterbi_chunk", "pd_f0_align"):
        assert name in _lib.EXPORTS
        getattr(lib, name)
    assert lib.pd_rmvpe_viterbi_chunk() == RM.VITERBI_CHUNK
    for name in ("viterbi_path", "to_viterbi_f0", "align_f0"):
        assert getattr(prodiff_amd, name) is getattr(RM, name) and name in prodiff_amd.__all__
    assert callable(RM.RMVPE.get_pitch_batch)


def test_host_tensors_are_refused():
    with pytest.raises(NotImplementedError):
        RM.RMVPE.decode(None, torch.zeros(1, 4, 360), use_viterbi=True)
    with pytest.raises(_lib.HipError):
        RM.viterbi_path(torch.zeros(1, 4, 360))
    with pytest.raises(_lib.HipError):
        RM.align_f0(torch.zeros(1, 4), 0.01, 0.0116, 3)
