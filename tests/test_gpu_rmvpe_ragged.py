"""GPU tests of the ragged RMVPE path (pd_rmvpe_forward_ragged, pd_rmvpe_viterbi_ragged, pd_f0_align_ragged and
``RMVPE.get_pitch_batch`` on clips of different lengths).

The bar is exactness: the library guarantees that a row's result depends neither on B nor on its batch position
(tests/test_gpu_rmvpe.py, tests/test_gpu_viterbi.py), so a row of a ragged batch must equal, bit for bit
(``torch.equal``), the same clip run alone through the equal-length entry points, which the fixtures pin to the
reference.  One test compares the ragged call with the reference's own outputs directly, under the bars of
tests/test_gpu_rmvpe.py::test_parity_with_the_reference.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from prodiff_amd import _lib, synth
from prodiff_amd import rmvpe as RM
from tests import rmvpe_cases as RC
from tests import viterbi_ref as V
from tests.test_gpu_rmvpe import case_net, extractor, fixture

pytestmark = pytest.mark.gpu

CH = RM.VITERBI_CHUNK
# name -> (the case of tests/rmvpe_cases.py whose network it runs, frames per row, input seed)
SETS = {
    "shallow": ("rmvpe_shallow", (20, 9, 3), 301),          # image heights 20, 12 and 4 against 8-row tiles
    "slim": ("rmvpe_slim", (64, 33, 32, 1), 302),           # bottom maps of 2, 2, 1 and 1 rows
    "full": ("rmvpe_full_b2t64", (96, 40, 64), 303),
    "nogru": ("rmvpe_nogru", (40, 17), 304),
}


def cuda(x):
    return torch.from_numpy(np.array(x)).cuda()          # a copy: the shared inputs are read-only


def unit_of(case):
    return 1 << RC.CASES[case][0]["en_de_layers"]


def padded(frames, unit):
    return -(-max(frames) // unit) * unit


@functools.lru_cache(maxsize=None)
def set_mel(name):
    """The set's time-major input [B, T, 128], T the longest row padded to 2^levels; never modified."""
    case, frames, seed = SETS[name]
    mel = synth.synth_inputs(seed, (len(frames), padded(frames, unit_of(case)), RC.N_MELS), loc=-4.0, scale=2.0)
    mel.setflags(write=False)
    return mel


def single_run(net, row, n, unit):
    """The first n frames of ``row`` [T, 128] alone: zero-padded to the unit, as RMVPE.mel2hidden pads -> (hidden, feat)"""
    x = np.zeros((1, padded((n,), unit), RC.N_MELS), np.float32)
    x[0, :n] = row[:n]
    hidden, feat = net.forward_time_major(cuda(x), return_feat=True)
    return hidden[0, :n], feat[0, :n]


@functools.lru_cache(maxsize=None)
def singles(name):
    case, frames, _ = SETS[name]
    net = case_net(case)
    return [single_run(net, set_mel(name)[b], n, unit_of(case)) for b, n in enumerate(frames)]


def check_rows(hidden, feat, frames, want, order=None):
    for row, b in enumerate(order if order is not None else range(len(frames))):
        n = frames[b]
        assert torch.isfinite(hidden[row, :n]).all() and torch.isfinite(feat[row, :n]).all(), row
        assert torch.equal(hidden[row, :n], want[b][0]), (row, "hidden")
        assert torch.equal(feat[row, :n], want[b][1]), (row, "feat")


# ---------------------------------------------------------------- the network
@pytest.mark.parametrize("name", list(SETS))
def test_network_rows_equal_their_single_runs(name):
    case, frames, _ = SETS[name]
    hidden, feat = case_net(case).forward_time_major(cuda(set_mel(name)), return_feat=True, frames=list(frames))
    assert hidden.shape[:2] == feat.shape[:2] == set_mel(name).shape[:2]
    check_rows(hidden, feat, frames, singles(name))


@pytest.mark.parametrize("name", ["shallow", "slim"])
def test_padding_is_never_read(name):
    case, frames, _ = SETS[name]
    net = case_net(case)
    mel = set_mel(name).copy()
    for b, n in enumerate(frames):
        mel[b, n:] = np.nan
    hidden, feat = net.forward_time_major(cuda(mel), return_feat=True, frames=list(frames))
    check_rows(hidden, feat, frames, singles(name))
    order = list(range(len(frames)))[::-1]
    hidden, feat = net.forward_time_major(cuda(mel[order]), return_feat=True, frames=[frames[b] for b in order])
    check_rows(hidden, feat, frames, singles(name), order)


def test_more_rows_than_one_recurrence_block_with_mixed_lengths():
    """18 rows: the second recurrence block holds two rows, the first holds every length."""
    net = case_net("rmvpe_shallow")
    B, cycle = 18, (20, 9, 3, 16)
    frames = [cycle[b % 4] for b in range(B)]
    mel = synth.synth_inputs(305, (B, 20, RC.N_MELS), loc=-4.0, scale=2.0)
    want = [single_run(net, mel[b], frames[b], 4) for b in range(B)]
    hidden, feat = net.forward_time_major(cuda(mel), return_feat=True, frames=frames)
    check_rows(hidden, feat, frames, want)


def test_parity_with_the_reference_on_a_ragged_batch():
    """rmvpe_full_b2t64 and rmvpe_full_b1t96 (one parameter seed) as one batch of 64, 64 and 96 frames, against the
    fixtures' reference outputs under test_parity_with_the_reference's bars:
    hidden max|d| <= 1e-4, feat max|d| <= 1e-4 max|reference feat|, e_hip <= 8 e_ref + 1e-6 against float64."""
    a, c = fixture("rmvpe_full_b2t64"), fixture("rmvpe_full_b1t96")
    assert RC.CASES["rmvpe_full_b2t64"][3] == RC.CASES["rmvpe_full_b1t96"][3]
    mel = np.full((3, 96, RC.N_MELS), np.nan, np.float32)
    mel[:2, :64] = a["mel"].transpose(0, 2, 1)
    mel[2] = c["mel"][0].T
    hidden, feat = case_net("rmvpe_full_b2t64").forward_time_major(cuda(mel), return_feat=True, frames=[64, 64, 96])
    hidden, feat = hidden.cpu().numpy(), feat.cpu().numpy()
    for d, got in ((a, {"hidden": hidden[:2, :64], "feat": feat[:2, :64]}), (c, {"hidden": hidden[2:], "feat": feat[2:]})):
        assert got["hidden"].shape == d["hidden"].shape and got["feat"].shape == d["feat"].shape
        assert np.isfinite(got["hidden"]).all() and np.isfinite(got["feat"]).all()
        peak = float(np.abs(d["feat"]).max())
        dh, df = float(np.abs(got["hidden"] - d["hidden"]).max()), float(np.abs(got["feat"] - d["feat"]).max())
        print(f"ragged rows of {d['hidden'].shape}: hidden max|d| = {dh:.2e}, feat max|d| / peak = {df / peak:.2e}")
        assert dh <= 1e-4
        assert df <= 1e-4 * peak
        for key in ("hidden", "feat"):
            e_ref = float(np.abs(d[key] - d[key + "64"]).max())
            assert float(np.abs(got[key] - d[key + "64"]).max()) <= 8 * e_ref + 1e-6, key


# ---------------------------------------------------------------- Viterbi
def check_viterbi(h, frames, w):
    T = h.shape[1]
    path, logp = RM.viterbi_path(cuda(h), width=w, return_logp=True, frames=list(frames))
    assert path.shape == (len(frames), T) and path.dtype == torch.int64
    for b, n in enumerate(frames):
        p1, l1 = RM.viterbi_path(cuda(h[b:b + 1, :n]), width=w, return_logp=True)
        assert torch.equal(path[b, :n], p1[0]), b
        assert torch.equal(logp[b], l1[0]), b
        assert not path[b, n:].any(), b
    filled = h.copy()
    for b, n in enumerate(frames):
        filled[b, n:] = np.nan
    path2, logp2 = RM.viterbi_path(cuda(filled), width=w, return_logp=True, frames=list(frames))
    assert torch.equal(path2, path) and torch.equal(logp2, logp)


def test_viterbi_rows_equal_their_single_runs():
    T = 2 * CH + 6
    frames = (1, CH - 1, CH, CH + 1, T)                   # either side of the chunk of 32 frames
    assert frames == (1, 31, 32, 33, 70)
    check_viterbi(np.stack([V.case(name, T) for name in V.CASE_NAMES]), frames, V.WIDTH)


def test_viterbi_small_state_space():
    T = 2 * CH + 1
    check_viterbi(np.stack([V.case(name, T, 40) for name in ("rand", "glide", "jump")]), (T, CH + 1, 7), 5)


# ---------------------------------------------------------------- align
ALIGN_ROWS = (("voiced", 2, 1), ("unvoiced", 51, 17), ("runs", 101, 87), ("single", 64, 120))


@pytest.mark.parametrize("interp_uv", [False, True])
def test_align_rows_equal_their_single_runs(interp_uv):
    """(n, length) = (2, 1), (51, 17): cut; (101, 87): the last frames unvoiced; (64, 120): padded with the last value."""
    t_src, t_dst = 0.01, 512 / 44100
    rows = [V.f0_rows(n)[name] for name, n, _ in ALIGN_ROWS]
    assert not rows[1].any() and not rows[2][-5:].any()
    ns, lengths = [n for _, n, _ in ALIGN_ROWS], [ln for _, _, ln in ALIGN_ROWS]
    ms = [RM.resampled_length(n, t_src, t_dst) for n in ns]
    assert ms[1] > lengths[1] and ms[3] < lengths[3]       # a cut and a pad
    f0 = np.full((len(rows), max(ns)), 777.0, np.float32)  # a voiced value where nothing may be read
    for b, row in enumerate(rows):
        f0[b, :ns[b]] = row
    out, uv = RM.align_f0(cuda(f0), t_src, t_dst, lengths, interp_uv=interp_uv, frames=ns)
    assert out.shape == uv.shape == (len(rows), max(lengths)) and uv.dtype == torch.bool
    for b, row in enumerate(rows):
        o1, u1 = RM.align_f0(cuda(row[None]), t_src, t_dst, lengths[b], interp_uv=interp_uv)
        assert torch.equal(out[b, :lengths[b]], o1[0]) and torch.equal(uv[b, :lengths[b]], u1[0]), b
        assert not out[b, lengths[b]:].any() and uv[b, lengths[b]:].all(), b
    assert uv[1].all() and not uv[0, :1].any()


# ---------------------------------------------------------------- end to end
CLIPS = ((0.5, dict()), (0.31, dict(f_start=330.0, f_end=240.0, seed=8)), (0.2, dict(f_start=200.0, f_end=150.0, seed=9)))


@functools.lru_cache(maxsize=None)
def clips():
    return [RC.harmonic_signal(44100, sec, **kw) for sec, kw in CLIPS]


@functools.lru_cache(maxsize=None)
def alone(use_viterbi):
    lengths = clip_lengths()
    return [extractor().get_pitch_batch(w[None], 44100, lengths[b], hop_size=512, use_viterbi=use_viterbi)
            for b, w in enumerate(clips())]


def clip_lengths():
    return [int(round(len(w) / 512)) + 2 for w in clips()]


def check_pitch(got, use_viterbi):
    f0, uv = got
    lengths = clip_lengths()
    assert f0.is_cuda and f0.shape == uv.shape == (3, max(lengths)) and uv.dtype == torch.bool
    for b, (f1, u1) in enumerate(alone(use_viterbi)):
        assert torch.equal(f0[b, :lengths[b]], f1[0]) and torch.equal(uv[b, :lengths[b]], u1[0]), b
        assert not f0[b, lengths[b]:].any() and uv[b, lengths[b]:].all(), b
    assert (f0 > 0).any()


@pytest.mark.parametrize("use_viterbi", [False, True])
def test_get_pitch_batch_on_a_list_of_clips(use_viterbi):
    pe = extractor()
    check_pitch(pe.get_pitch_batch(clips(), 44100, clip_lengths(), hop_size=512, use_viterbi=use_viterbi), use_viterbi)


def test_get_pitch_batch_on_a_padded_tensor_with_lens():
    lens = [len(w) for w in clips()]
    wav = np.full((3, max(lens) + 100), 0.25, np.float32)      # the padding holds a signal that must not be heard
    for b, w in enumerate(clips()):
        wav[b, :lens[b]] = w
    pe = extractor()
    check_pitch(pe.get_pitch_batch(wav, 44100, clip_lengths(), lens=lens, hop_size=512), False)
    check_pitch(pe.get_pitch_batch(cuda(wav), 44100, clip_lengths(), lens=lens, hop_size=512), False)


def test_get_pitch_batch_refuses_a_row_that_is_too_short():
    with pytest.raises(ValueError, match="row 1"):
        extractor().get_pitch_batch([clips()[0], clips()[0][:400]], 44100, 40, hop_size=512)


# ---------------------------------------------------------------- graph
def test_graph_replay_equals_the_eager_chain():
    pe = extractor()
    frames = [70, 40]
    mel = cuda(synth.synth_inputs(306, (2, 70, RC.N_MELS), loc=-4.0, scale=2.0))
    t_dst = 512 / 44100
    triples = RM.align_rows(frames, [62, 30], 0.01, t_dst)
    fr = torch.tensor(frames, dtype=torch.int32, device="cuda")
    rows = torch.tensor(triples, dtype=torch.int32, device="cuda")

    def chain():
        hidden = pe._hidden_time_major(mel, frames=fr)
        path = RM.viterbi_path(hidden, frames=fr)
        f0 = RM.to_viterbi_f0(hidden, thred=0.03, frames=fr)
        return (path,) + RM.align_f0(f0, 0.01, t_dst, 62, frames=rows)

    eager = [x.clone() for x in chain()]
    want = RM.align_f0(RM.to_viterbi_f0(pe._hidden_time_major(mel, frames=frames), frames=frames), 0.01, t_dst, [62, 30],
                       frames=frames)
    assert torch.equal(eager[1], want[0]) and torch.equal(eager[2], want[1])      # device and host lengths agree
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


# ---------------------------------------------------------------- contract
def test_arguments_and_no_allocation():
    L = _lib.lib()
    net = case_net("rmvpe_slim")
    h = net.handle()
    B, T = 2, 64
    mel = torch.zeros(B, T + 1, 128, device="cuda")
    hidden = torch.empty(B, T + 1, 360, device="cuda")
    fr = torch.tensor([40, 64], dtype=torch.int32, device="cuda")
    need = L.pd_rmvpe_workspace_size(h, B, T)
    ws = torch.empty(need + 4096, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    live = L.pd_live_device_bytes()

    def call(frames=fr, T=T, nbytes=need):
        return L.pd_rmvpe_forward_ragged(h, _lib.fptr(mel), None if frames is None else frames.data_ptr(), _lib.fptr(hidden),
                                         None, B, T, C.c_void_p(ws.data_ptr()), nbytes, _lib.stream_ptr())

    assert call(frames=None) == 1 and b"null" in L.pd_last_error()                       # PD_ERR_ARG
    assert call(T=T + 1, nbytes=ws.numel()) == 1                                         # not a multiple of 2^levels
    assert call(nbytes=need - 1) == 3                                                    # PD_ERR_WORKSPACE
    assert call() == 0
    torch.cuda.synchronize()
    assert L.pd_live_device_bytes() == live
    x = torch.zeros(B, T, 128, device="cuda")
    for bad in ([40], [40, 64, 64], [0, 64], [40, T + 1]):
        with pytest.raises(_lib.HipError):
            net.forward_time_major(x, frames=bad)
    with pytest.raises(_lib.HipError):
        net.forward_time_major(torch.zeros(B, T + 1, 128, device="cuda"), frames=[40, 64])
    # the tail's entries
    sal = cuda(np.stack([V.case("rand", CH + 3), V.case("jump", CH + 3)]))
    RM.viterbi_path(sal)                                   # builds the cached tables
    band = RM._VITERBI_TABLES[(V.N_CLASS, V.WIDTH, str(sal.device))][0]
    _, log_off, log_init = RM.viterbi_tables(V.N_CLASS, V.WIDTH)
    path = torch.empty(2, CH + 3, device="cuda", dtype=torch.int64)
    vneed = L.pd_rmvpe_viterbi_workspace_size(2, CH + 3, V.N_CLASS, V.WIDTH)
    vws = torch.empty(vneed, dtype=torch.uint8, device="cuda")
    fr2 = torch.tensor([5, CH + 3], dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    live = L.pd_live_device_bytes()

    def vcall(frames):
        return L.pd_rmvpe_viterbi_ragged(sal.data_ptr(), band.data_ptr(), log_off, log_init, path.data_ptr(), None,
                                         None if frames is None else frames.data_ptr(), 2, CH + 3, V.N_CLASS, V.WIDTH,
                                         vws.data_ptr(), vneed, _lib.stream_ptr())

    assert vcall(None) == 1 and vcall(fr2) == 0
    f0 = torch.ones(2, 8, device="cuda")
    out = torch.empty(2, 4, device="cuda")
    uv = torch.empty(2, 4, device="cuda", dtype=torch.bool)
    rows = torch.tensor([[8, 7, 4], [3, 2, 2]], dtype=torch.int32, device="cuda")

    def acall(r=rows, n_stride=8):
        return L.pd_f0_align_ragged(f0.data_ptr(), out.data_ptr(), uv.data_ptr(), None if r is None else r.data_ptr(), 2,
                                    n_stride, 4, 0.01, 0.0116, 0, _lib.stream_ptr())

    assert acall(r=None) == 1 and acall(n_stride=1) == 1 and acall() == 0
    torch.cuda.synchronize()
    assert L.pd_live_device_bytes() == live
    for bad_frames, bad_length in (([8], [4, 4]), ([8, 1], [4, 4]), ([8, 9], [4, 4]), ([8, 8], [4, 0]), ([8, 8], [4])):
        with pytest.raises((ValueError, _lib.HipError)):
            RM.align_f0(f0, 0.01, 0.0116, bad_length, frames=bad_frames)
    with pytest.raises(_lib.HipError):
        RM.viterbi_path(sal, frames=[5, CH + 4])
