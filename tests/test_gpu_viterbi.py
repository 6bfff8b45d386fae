"""GPU tests of the native Viterbi decode (pd_rmvpe_viterbi) and f0 tail (pd_f0_align) against the float64
restatement tests/viterbi_ref.py.

Bars:
  path   exactly the dense restatement's (tests/test_viterbi_cpu.py shows that every case's path survives 1e-6
         relative noise on the log-probabilities; the kernel's differ from numpy's by double rounding only)
  logp   |native - ref| <= 1e-9 |ref|: the differences are double roundings of the sum and the log, about
         1e-16 T |lp|; the bound leaves three orders of margin
  f0     relative 4e-6 on the aligned curve: float32 log2 and exp2 on both sides, <= 2 ulp each at |log2 f0| < 16,
         one ulp of log2 f0 being 9.5e-7 ln 2 in f0; uv exactly
"""
import functools

import numpy as np
import pytest
import torch

from prodiff_amd import _lib
from prodiff_amd import rmvpe as RM
from tests import rmvpe_cases as RC
from tests import rmvpe_ref as R
from tests import viterbi_ref as V

pytestmark = pytest.mark.gpu

CH = RM.VITERBI_CHUNK
LENGTHS = (1, 2, 3, CH - 1, CH, CH + 1, 2 * CH + 1, 300)


def cuda(x):
    return torch.from_numpy(np.array(x)).cuda()          # a copy: the shared references are read-only


@functools.lru_cache(maxsize=None)
def reference(name, T, n=V.N_CLASS, w=V.WIDTH):
    """(hidden float32 [T, n], path, logp) of the dense restatement; computed once, never modified."""
    h = V.case(name, T, n)
    val, path = V.dense(h, w)
    h.setflags(write=False)
    path.setflags(write=False)
    return h, path, float(val[-1, path[-1]])


def run(h, w=V.WIDTH):
    path, logp = RM.viterbi_path(cuda(h), width=w, return_logp=True)
    return path.cpu().numpy(), logp.cpu().numpy()


def check_parity(name, T, n=V.N_CLASS, w=V.WIDTH):
    h, ref_path, ref_logp = reference(name, T, n, w)
    path, logp = run(h[None], w)
    assert path.shape == (1, T) and path.dtype == np.int64
    wrong = int((path[0] != ref_path).sum())
    rel = abs(logp[0] - ref_logp) / abs(ref_logp)
    print(f"{name} T = {T} n = {n} w = {w}: {wrong} frames differ, logp relative error {rel:.2e}")
    assert wrong == 0
    assert rel <= 1e-9


# ---------------------------------------------------------------- path parity
@pytest.mark.parametrize("name", V.CASE_NAMES)
def test_path_equals_the_dense_restatement(name):
    for T in LENGTHS:
        check_parity(name, T)


@pytest.mark.parametrize("n,w", [(40, 5), (8, 30), (100, 40)])
def test_small_state_spaces(n, w):
    """n = 40, w = 5: the band edges dominate; n = 8, w = 30: every state lies in every band, the out-of-band
    candidate is never used; n = 100, w = 40: a band wider than the kernel keeps in registers."""
    for name in ("rand", "glide", "jump"):
        check_parity(name, 2 * CH + 1, n, w)


def test_rows_equal_their_single_runs():
    T = 2 * CH + 1
    hs = np.stack([reference(name, T)[0] for name in ("rand", "jump", "uniform")])
    path, logp = run(hs)
    for b in range(3):
        p1, l1 = run(hs[b:b + 1])
        assert np.array_equal(path[b], p1[0]) and logp[b] == l1[0], b
        assert np.array_equal(path[b], reference(("rand", "jump", "uniform")[b], T)[1])


def test_an_all_zero_frame_counts_as_uniform():
    """The reference divides by the frame's sum there and yields NaN; the native rule is p = 1 / n for that frame."""
    T = CH + 8
    h = np.stack([reference("rand", T)[0], reference("glide", T)[0]]).copy()
    h[0, 7] = 0.0
    path, logp = run(h)
    assert path.min() >= 0 and path.max() < V.N_CLASS and np.isfinite(logp).all()
    assert np.array_equal(path[1], reference("glide", T)[1])
    same = h[0].copy()
    same[7] = 1.0                                         # any constant frame normalises to 1 / n
    val, ref = V.dense(same)
    assert np.array_equal(path[0], ref)
    assert abs(logp[0] - val[-1, ref[-1]]) <= 1e-9 * abs(val[-1, ref[-1]])


# ---------------------------------------------------------------- to_viterbi_f0
def test_to_viterbi_f0():
    T = 2 * CH + 1
    names = ("rand", "glide")
    hs = np.stack([reference(name, T)[0] for name in names])
    paths = np.stack([reference(name, T)[1] for name in names])
    thred = 0.03
    f64 = R.local_average_f0(hs, thred, paths)
    f0 = RM.to_viterbi_f0(cuda(hs), thred=thred)
    assert f0.is_cuda and f0.shape == (2, T)
    f0 = f0.cpu().numpy()
    voiced = f64 > 0
    assert voiced.all()
    rel = np.abs(f0 - f64) / f64
    print(f"to_viterbi_f0: max relative error {float(rel.max()):.2e}")
    assert rel.max() <= 1e-6
    # on random saliences the path is not the frame-wise argmax: a decode that ignored the path would not pass
    plain = RM.to_local_average_f0(cuda(hs), thred=thred).cpu().numpy()
    assert (paths[0] != hs[0].argmax(-1)).mean() > 0.9
    assert (np.abs(plain[0] - f0[0]) > 1e-3 * f0[0]).mean() > 0.9


# ---------------------------------------------------------------- align_f0
@pytest.mark.parametrize("n", [2, 3, 101, 1001])
def test_align_f0(n):
    rows = V.f0_rows(n)
    f0 = cuda(np.stack(list(rows.values())))
    worst = 0.0
    for t_src, t_dst in V.GRIDS:
        m = RM.resampled_length(n, t_src, t_dst)
        assert m == len(np.arange(0, (n - 1) * t_src, t_dst))
        for length in sorted({max(m - 1, 1), m, m + 3}):
            for interp_uv in (False, True):
                out, uv = RM.align_f0(f0, t_src, t_dst, length, interp_uv=interp_uv)
                assert out.shape == uv.shape == (len(rows), length) and uv.dtype == torch.bool and out.is_cuda
                out, uv = out.cpu().numpy(), uv.cpu().numpy()
                for b, (name, row) in enumerate(rows.items()):
                    ref, ref_uv = V.align_f0(row, t_src, t_dst, length, interp_uv)
                    assert np.array_equal(uv[b], ref_uv), (name, t_dst, length, interp_uv)
                    zero = ref == 0
                    assert (out[b][zero] == 0).all(), (name, t_dst, length, interp_uv)
                    if (~zero).any():
                        rel = float((np.abs(out[b] - ref)[~zero] / ref[~zero]).max())
                        worst = max(worst, rel)
                        assert rel <= 4e-6, (name, t_dst, length, interp_uv, rel)
    print(f"align_f0 n = {n}: max relative error {worst:.2e}")


def test_align_f0_refuses_curves_it_cannot_resample():
    with pytest.raises(ValueError):
        RM.align_f0(torch.ones(1, 1, device="cuda"), 0.01, 512 / 44100, 4)
    with pytest.raises(ValueError):
        RM.align_f0(torch.ones(1, 8, device="cuda"), 0.01, 512 / 44100, 0)
    out, uv = RM.align_f0(torch.full((9,), 220.0, device="cuda"), 0.01, 512 / 44100, 5)      # a single curve
    assert out.shape == uv.shape == (5,) and not uv.any()


# ---------------------------------------------------------------- get_pitch_batch
def extractor():
    from tests.test_gpu_rmvpe import extractor as shared      # one full-size synthetic network per session
    return shared()


@pytest.mark.parametrize("sr,hop", [(16000, 128), (44100, 512)])
def test_get_pitch_batch(sr, hop):
    pe = extractor()
    wav = np.stack([RC.harmonic_signal(sr, 0.5), RC.harmonic_signal(sr, 0.5, f_start=330.0, f_end=240.0, seed=8)])
    length = int(round(0.5 * sr / hop)) + 2
    for interp_uv in (False, True):
        f0, uv = pe.get_pitch_batch(wav, sr, length, hop_size=hop, interp_uv=interp_uv)
        assert f0.is_cuda and uv.is_cuda and f0.shape == uv.shape == (2, length) and uv.dtype == torch.bool
        f0, uv = f0.cpu().numpy(), uv.cpu().numpy()
        for b in range(2):
            ref, ref_uv = pe.get_pitch(wav[b], sr, length, hop_size=hop, interp_uv=interp_uv)
            assert np.array_equal(uv[b], ref_uv), (b, interp_uv)
            both = (ref != 0) & (f0[b] != 0)
            assert np.array_equal(ref == 0, f0[b] == 0)
            if both.any():
                assert (np.abs(f0[b] - ref)[both] / ref[both]).max() <= 4e-6
    # device waveforms give the same tensors
    f0_d, uv_d = pe.get_pitch_batch(cuda(wav), sr, length, hop_size=hop, interp_uv=True)
    assert np.array_equal(f0_d.cpu().numpy(), f0) and np.array_equal(uv_d.cpu().numpy(), uv)
    # Viterbi: the chain step by step
    hidden = pe._hidden_from_audio(cuda(wav), sr)
    want = RM.align_f0(RM.to_viterbi_f0(hidden, thred=0.03), 0.01, hop / sr, length, interp_uv=False)
    got = pe.get_pitch_batch(wav, sr, length, hop_size=hop, use_viterbi=True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    ref, ref_uv = pe.get_pitch(wav[1], sr, length, hop_size=hop, use_viterbi=True)
    assert np.array_equal(got[1][1].cpu().numpy(), ref_uv)


def test_decode_with_viterbi_on_a_device_tensor():
    T = CH + 1
    h, path, _ = reference("glide", T)
    f0 = RM.RMVPE.decode(None, cuda(h[None]), thred=0.03, use_viterbi=True)
    f64 = R.local_average_f0(h, 0.03, path)
    assert isinstance(f0, np.ndarray) and f0.shape == (T,)
    assert (np.abs(f0 - f64) <= 1e-6 * f64).all()


# ---------------------------------------------------------------- contract
def test_return_codes_and_no_allocation():
    L = _lib.lib()
    B, T, n, w = 2, CH + 3, V.N_CLASS, V.WIDTH
    h = cuda(np.stack([reference("rand", T)[0], reference("jump", T)[0]]))
    RM.viterbi_path(h)                                    # builds the cached tables
    band = RM._VITERBI_TABLES[(n, w, str(h.device))][0]
    _, log_off, log_init = RM.viterbi_tables(n, w)
    path = torch.empty(B, T, device="cuda", dtype=torch.int64)
    need = L.pd_rmvpe_viterbi_workspace_size(B, T, n, w)
    assert need > 0 and L.pd_rmvpe_viterbi_workspace_size(B, T, 2048, w) == 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    live = L.pd_live_device_bytes()

    def call(hid=h, bnd=band, out=path, B=B, T=T, n=n, w=w, nbytes=need):
        return L.pd_rmvpe_viterbi(None if hid is None else hid.data_ptr(), None if bnd is None else bnd.data_ptr(), log_off,
                                  log_init, None if out is None else out.data_ptr(), None, B, T, n, w, ws.data_ptr(), nbytes,
                                  _lib.stream_ptr())

    assert call(hid=None) == 1 and call(bnd=None) == 1 and call(out=None) == 1          # PD_ERR_ARG
    assert call(B=0) == 1 and call(T=0) == 1
    assert call(n=2048) == 4 and call(w=65) == 4                                         # PD_ERR_UNSUPPORTED
    assert call(nbytes=need - 1) == 3                                                    # PD_ERR_WORKSPACE
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(path.cpu().numpy()[1], reference("jump", T)[1])
    f0 = torch.ones(1, 8, device="cuda")
    out = torch.empty(1, 4, device="cuda")
    uv = torch.empty(1, 4, device="cuda", dtype=torch.bool)
    args = (f0.data_ptr(), out.data_ptr(), uv.data_ptr(), 1)
    assert L.pd_f0_align(*args, 1, 4, 4, 0.01, 0.0116, 0, _lib.stream_ptr()) == 1        # n < 2
    assert L.pd_f0_align(*args, 8, 0, 4, 0.01, 0.0116, 0, _lib.stream_ptr()) == 1        # m < 1
    assert L.pd_f0_align(None, out.data_ptr(), uv.data_ptr(), 1, 8, 4, 4, 0.01, 0.0116, 0, _lib.stream_ptr()) == 1
    assert L.pd_f0_align(*args, 8, 4, 4, 0.01, 0.0116, 0, _lib.stream_ptr()) == 0
    RM.align_f0(f0, 0.01, 0.0116, 4)
    torch.cuda.synchronize()
    assert L.pd_live_device_bytes() == live


def test_graph_replay_equals_the_eager_chain():
    T = 2 * CH + 1
    quiet = reference("zeros", T)[0].copy()
    quiet[10:25] *= 0.2                                   # frames below the threshold: unvoiced
    h = cuda(np.stack([reference("rand", T)[0], quiet]))

    def chain():
        path = RM.viterbi_path(h)
        f0 = RM.to_local_average_f0(h, center=path, thred=0.5)
        return (path,) + RM.align_f0(f0, 0.01, 512 / 44100, 60)

    eager = [x.clone() for x in chain()]
    assert eager[2].any() and not eager[2].all()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = chain()
    for x in outs:
        x.zero_()
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(outs, eager):
        assert torch.equal(a, b)
