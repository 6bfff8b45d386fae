"""GPU tests of the native RMVPE pitch extractor (pd_rmvpe, pd_rmvpe_decode, the centred pd_mel) against the
reference's own outputs (tests/golden/rmvpe_*.npz, made by tests/golden/gen_golden_rmvpe.py from
modules/rmvpe/model.py on the CPU) and the float64 restatement tests/rmvpe_ref.py.

Bars:
  hidden  max|native - reference f32| <= 1e-4 (the project's fp32 bar; the salience lies in [0, 1])
  feat    max|native - reference f32| <= 1e-4 * max|reference feat|
  f64     e_hip = max|native - f64| <= 8 e_ref + 1e-6, e_ref = max|reference f32 - f64| (test_gpu_mel.py's rule with
          the factor doubled for the BatchNorm fold's extra rounding)
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import prodiff_amd
from prodiff_amd import _lib, synth
from prodiff_amd import rmvpe as RM
from tests import golden_io
from tests import rmvpe_cases as RC
from tests import rmvpe_ref as R

pytestmark = pytest.mark.gpu


def cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


@functools.lru_cache(maxsize=None)
def host_params(model_items, seed):
    return synth.synth_rmvpe_params(synth.rmvpe_param_shapes(**dict(model_items)), seed)


@functools.lru_cache(maxsize=None)
def net_of(model_items, seed):
    """One native model per (architecture, seed) for the whole session."""
    model = dict(model_items)
    net = prodiff_amd.E2E0(model["n_blocks"], model["n_gru"], (2, 2), model["en_de_layers"], model["inter_layers"], 1,
                           model["en_out_channels"])
    net.load_state_dict({k: torch.from_numpy(v) for k, v in host_params(model_items, seed).items()})
    return net.cuda()


def case_net(name):
    model, _, _, pseed, _ = RC.CASES[name]
    return net_of(tuple(sorted(model.items())), pseed)


@functools.lru_cache(maxsize=None)
def fixture(name):
    return golden_io.load(name)


# ---------------------------------------------------------------- parity
@pytest.mark.parametrize("name", list(RC.CASES))
def test_parity_with_the_reference(name):
    d = fixture(name)
    hidden, feat = case_net(name).forward_features(cuda(d["mel"]))
    hidden, feat = hidden.cpu().numpy(), feat.cpu().numpy()
    assert hidden.shape == d["hidden"].shape and feat.shape == d["feat"].shape
    assert np.isfinite(hidden).all() and np.isfinite(feat).all()
    peak = float(np.abs(d["feat"]).max())
    dh, df = float(np.abs(hidden - d["hidden"]).max()), float(np.abs(feat - d["feat"]).max())
    line = f"{name}: hidden max|d| = {dh:.2e}, feat max|d| / peak = {df / peak:.2e}"
    for key, x in (("hidden", hidden), ("feat", feat)):
        e_ref = float(np.abs(d[key] - d[key + "64"]).max())
        e_hip = float(np.abs(x - d[key + "64"]).max())
        line += f", {key}: e_ref = {e_ref:.2e} e_hip = {e_hip:.2e}"
    print(line)
    assert dh <= 1e-4
    assert df <= 1e-4 * peak
    for key, x in (("hidden", hidden), ("feat", feat)):
        e_ref = float(np.abs(d[key] - d[key + "64"]).max())
        assert float(np.abs(x - d[key + "64"]).max()) <= 8 * e_ref + 1e-6, key


def test_forward_equals_forward_features():
    d = fixture("rmvpe_shallow")
    net = case_net("rmvpe_shallow")
    hidden, _ = net.forward_features(cuda(d["mel"]))
    assert torch.equal(net(cuda(d["mel"])), hidden)


# ---------------------------------------------------------------- batch independence
@pytest.mark.parametrize("name", ["rmvpe_shallow", "rmvpe_slim", "rmvpe_full_b2t64"])
def test_rows_equal_their_single_runs(name):
    d = fixture(name)
    net = case_net(name)
    hidden, feat = net.forward_features(cuda(d["mel"]))
    for b in range(d["mel"].shape[0]):
        h1, f1 = net.forward_features(cuda(d["mel"][b:b + 1]))
        assert torch.equal(h1[0], hidden[b]) and torch.equal(f1[0], feat[b]), b


def test_a_row_does_not_depend_on_its_batch_position():
    d = fixture("rmvpe_full_b1t96")
    net = case_net("rmvpe_full_b1t96")
    h1, f1 = net.forward_features(cuda(d["mel"]))
    h2, f2 = net.forward_features(cuda(np.concatenate([d["mel"], d["mel"]])))
    for b in range(2):
        assert torch.equal(h2[b], h1[0]) and torch.equal(f2[b], f1[0]), b


def test_more_rows_than_one_recurrence_block():
    """17 rows: the GRU's second group of 16 batch rows holds a single row."""
    d = fixture("rmvpe_shallow")
    net = case_net("rmvpe_shallow")
    alone = [net.forward_features(cuda(d["mel"][b:b + 1])) for b in range(2)]
    order = [0, 1, 1, 0, 1] * 3 + [0, 1]
    hidden, feat = net.forward_features(cuda(d["mel"][order]))
    for row, b in enumerate(order):
        assert torch.equal(hidden[row], alone[b][0][0]) and torch.equal(feat[row], alone[b][1][0]), row


# ---------------------------------------------------------------- decode
def check_decode(hidden, thred, center=None):
    f64 = R.local_average_f0(hidden, thred, center)
    f0 = RM.to_local_average_f0(cuda(hidden), None if center is None else cuda(center), thred).cpu().numpy()
    voiced = f64 > 0
    assert voiced.any() and (~voiced).any()
    assert (f0[~voiced] == 0).all()
    rel = np.abs(f0[voiced] - f64[voiced]) / f64[voiced]
    print(f"decode: {int(voiced.sum())} voiced of {voiced.size}, max relative error {float(rel.max()):.2e}")
    assert rel.max() <= 1e-6


def test_decode_hand_built_frames():
    h = R.decode_cases()[None]
    check_decode(h, 0.03)
    f0 = RM.to_local_average_f0(cuda(h), thred=0.03).cpu().numpy()[0]
    assert f0[4] == 0 and f0[5] == 0                       # all-zero frame, maximum below thred
    f_tie = R.local_average_f0(h[0, 6], 0.0, center=np.int64(100))
    assert abs(f0[6] - f_tie) <= 1e-6 * f_tie              # the tie resolves to the lowest index


def test_decode_golden_salience():
    hidden = fixture("rmvpe_full_b2t64")["hidden"]
    check_decode(hidden, float(np.median(hidden.max(-1))))


def test_decode_with_explicit_center():
    hidden = fixture("rmvpe_slim")["hidden"]
    rng = np.random.default_rng(5)
    center = rng.integers(-3, RC.N_CLASS + 3, hidden.shape[:2])      # clamped into [0, n_class)
    check_decode(hidden, float(np.median(hidden.max(-1))), center)


# ---------------------------------------------------------------- end to end
@functools.lru_cache(maxsize=None)
def extractor():
    pe = RM.RMVPE({})
    pe.model.load_state_dict({k: torch.from_numpy(v) for k, v in
                              host_params(tuple(sorted(RC.FULL.items())), RC.CASES["rmvpe_full_b2t64"][3]).items()})
    pe.model.cuda()
    return pe


def f0_chain64(audio, sr):
    """resampler, centred mel, network, decode in float64 -> (f0 [T], hidden [T, 360])"""
    from tests import resample_ref as RR
    x = np.asarray(audio, np.float64)[None]
    if sr != 16000:
        h, W, o, n = RR.table64(sr, 16000, lowpass_filter_width=128)
        x = RR.direct64(x, h.astype(np.float32).astype(np.float64), W, o, n)
    basis = prodiff_amd.mel_filterbank(16000, 1024, 128, 30, 8000, htk=True)
    logmel = R.centered_mel(x, basis)[2]                     # [1, T, 128]
    T = logmel.shape[1]
    pad = -T % 32
    mel = np.pad(logmel, ((0, 0), (0, pad), (0, 0))).transpose(0, 2, 1)
    P = host_params(tuple(sorted(RC.FULL.items())), RC.CASES["rmvpe_full_b2t64"][3])
    hidden = R.e2e0(P, RC.FULL, mel)[1][0, :T]
    return R.local_average_f0(hidden, 0.03), hidden


@pytest.mark.parametrize("sr", [16000, 44100])
def test_f0_from_audio(sr):
    audio = RC.harmonic_signal(sr, 0.5)
    f64, hidden = f0_chain64(audio, sr)
    f0 = extractor().infer_from_audio(audio, sample_rate=sr)
    n16 = len(audio) if sr == 16000 else -(-len(audio) * 160 // 441)      # ceil(n L / o) samples at 16 kHz
    assert f0.shape == f64.shape == (1 + n16 // 160,)
    top = np.sort(hidden, axis=-1)
    keep = top[:, -1] - top[:, -2] >= 2e-4
    assert keep.mean() >= 0.9, f"{1 - keep.mean():.1%} of the frames have a top-two margin below 2e-4"
    voiced = f64 > 0
    assert (f0[keep & ~voiced] == 0).all()
    rel = np.abs(f0 - f64)[keep & voiced] / f64[keep & voiced]
    print(f"f0 at {sr} Hz: {int(keep.sum())} of {keep.size} frames compared, {int(voiced.sum())} voiced, "
          f"max relative error {float(rel.max()) if rel.size else 0.0:.2e}")
    assert rel.size and rel.max() <= 1e-4


# ---------------------------------------------------------------- centred mel
@functools.lru_cache(maxsize=None)
def mel_extractor():
    return RM.MelSpectrogram(128, 16000, 1024, 160, None, 30, 8000)


@pytest.mark.parametrize("L", [513, 1024, 160 * 33 + 7])
def test_centred_mel(L):
    rng = np.random.default_rng(L)
    wav = np.stack([RC.harmonic_signal(16000, L / 16000.0)[:L], (0.1 * rng.standard_normal(L)).astype(np.float32)])
    ms = mel_extractor()
    spec64, _, mel64 = R.centered_mel(wav, ms.mel_basis_host.numpy())
    y = torch.from_numpy(wav)
    spec32 = torch.stft(y, 1024, hop_length=160, win_length=1024, window=torch.hann_window(1024), center=True,
                        return_complex=True).abs()
    mel32 = torch.log(torch.clamp(torch.matmul(ms.mel_basis_host, spec32), min=1e-5)).numpy().transpose(0, 2, 1)
    mel, spec = ms.forward_time_major(cuda(wav), return_spec=True)
    assert mel.shape == (2, 1 + L // 160, 128)
    assert torch.equal(ms(cuda(wav)), mel.transpose(1, 2))
    mel, spec = mel.cpu().numpy(), spec.cpu().numpy()
    peak = spec64.max(axis=2, keepdims=True)
    d_spec = np.abs(spec - spec64)
    e_ref, e_hip = float(np.abs(mel32 - mel64).max()), float(np.abs(mel - mel64).max())
    print(f"L = {L}: spectrum max|d| / frame peak = {float((d_spec / peak).max()):.2e}, e_ref = {e_ref:.2e}, "
          f"e_hip = {e_hip:.2e}")
    assert (d_spec <= 1e-5 * peak).all()
    assert e_hip <= 4 * e_ref + 2e-6


def test_a_centred_handle_leaves_the_plain_one_alone():
    s = prodiff_amd.STFT(16000, 128, 1024, 1024, 160, 30, 8000)
    wav = cuda(RC.harmonic_signal(16000, 0.3)[None])
    before = s.get_mel_time_major(wav).clone()
    ms = RM.MelSpectrogram(128, 16000, 1024, 160, None, 30, 8000)
    centred = ms.forward_time_major(wav)
    after = s.get_mel_time_major(wav)
    assert torch.equal(before, after)
    assert centred.shape[1] == 1 + wav.shape[1] // 160 and before.shape[1] == 1 + (wav.shape[1] - 160) // 160
    with pytest.raises(NotImplementedError):
        s.get_mel(wav, center=True)
    ms.close()
    s.close()


# ---------------------------------------------------------------- contract
def create_raw(dims, params, dtype=_lib.PD_DTYPE_F32):
    arr = (C.c_void_p * len(params))(*[p.data_ptr() for p in params])
    h = C.c_void_p()
    rc = _lib.lib().pd_rmvpe_create(C.byref(dims), arr, dtype, _lib.stream_ptr(), C.byref(h))
    return rc, h


def test_unsupported_and_bad_arguments():
    L = _lib.lib()
    net = case_net("rmvpe_slim")
    params = [p.detach().float().contiguous() for p in net.ordered_params()]
    live = L.pd_live_device_bytes()
    assert create_raw(net.dims(), params, _lib.PD_DTYPE_BF16)[0] == 4          # PD_ERR_UNSUPPORTED
    for field, value in (("n_gru", 2), ("en_out_channels", 8)):
        dims = net.dims()
        setattr(dims, field, value)
        assert create_raw(dims, params)[0] == 4, field
        assert L.pd_rmvpe_num_params(C.byref(dims)) == 0
    assert L.pd_live_device_bytes() == live
    h = net.handle()
    B, T = 1, 32
    mel = torch.zeros(B, T + 1, 128, device="cuda")
    hidden = torch.empty(B, T + 1, 360, device="cuda")
    ws = torch.empty(L.pd_rmvpe_workspace_size(h, B, T + 1) + 256, dtype=torch.uint8, device="cuda")
    args = (_lib.fptr(mel), _lib.fptr(hidden), None, B)
    assert L.pd_rmvpe_forward(h, *args, T + 1, C.c_void_p(ws.data_ptr()), ws.numel(), _lib.stream_ptr()) == 1   # PD_ERR_ARG
    need = L.pd_rmvpe_workspace_size(h, B, T)
    assert need > 0
    assert L.pd_rmvpe_forward(h, *args, T, C.c_void_p(ws.data_ptr()), need - 1, _lib.stream_ptr()) == 3        # PD_ERR_WORKSPACE
    assert L.pd_rmvpe_forward(h, *args, T, C.c_void_p(ws.data_ptr()), need, _lib.stream_ptr()) == 0
    torch.cuda.synchronize()


def test_close_returns_the_device_memory():
    L = _lib.lib()
    model = RC.CASES["rmvpe_shallow"][0]
    torch.cuda.synchronize()
    live = L.pd_live_device_bytes()
    net = prodiff_amd.E2E0(model["n_blocks"], model["n_gru"], (2, 2), model["en_de_layers"], model["inter_layers"], 1,
                           model["en_out_channels"])
    net.load_state_dict({k: torch.from_numpy(v) for k, v in RC.case_params("rmvpe_shallow").items()})
    net.cuda()
    net(cuda(RC.case_mel("rmvpe_shallow")))
    assert L.pd_live_device_bytes() > live
    net.close()
    assert L.pd_live_device_bytes() == live


def test_graph_replay_equals_the_eager_call():
    d = fixture("rmvpe_slim")
    net = case_net("rmvpe_slim")
    mel = cuda(d["mel"]).transpose(1, 2).contiguous()
    eager = net.forward_time_major(mel).clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = net.forward_time_major(mel)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
