"""GPU tests of the native harmonic-noise separation (pd_vr: STFT, CascadedNet mask, iSTFT) against the reference's own
outputs (tests/golden/vr_*.npz, made by tests/golden/gen_golden_vr.py from modules/vr/nets.py on the CPU).

Bars:
  stft   real and imaginary parts within 1e-5 of each frame's peak |spec| (test_gpu_mel.py's spectrum bar)
  mask   from the fixture's own reference spectrum: max|native - reference f32| <= 1e-4, and
         e_hip = max|native - f64| <= 8 e_ref + 1e-6, e_ref = max|reference f32 - f64| (test_gpu_rmvpe.py's rule)
  y      the inverse of the reference's spec * mask, and the whole predict_from_audio:
         max|native - reference f32| <= 1e-5 max|y_ref| (the project's waveform bar); e_hip and e_ref against the
         float64 run are printed, not asserted
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import prodiff_amd
from prodiff_amd import _lib
from prodiff_amd import vr as VR
from tests import golden_io
from tests import vr_cases as VC

pytestmark = pytest.mark.gpu


def cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


@functools.lru_cache(maxsize=None)
def net_of(args_items, seed):
    """One native model per (architecture, seed) for the whole session."""
    a = dict(args_items)
    net = prodiff_amd.CascadedNet(**a)
    P = VC.synth.synth_vr_params(VC.synth.vr_param_shapes(a["n_fft"], a["nout"], a["nout_lstm"], a["is_mono"]), seed)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
    return net.cuda()


def case_net(name):
    return net_of(tuple(sorted(VC.model_args(name).items())), VC.CASES[name][7])


@functools.lru_cache(maxsize=None)
def fixture(name):
    return golden_io.load(name)


def mask64_of(name, mask):
    d = fixture(name)
    return (mask if name in VC.SMALL else mask.reshape(-1)[d["mask64_pos"]]), \
        (d["mask"] if name in VC.SMALL else d["mask"].reshape(-1)[d["mask64_pos"]])


# ---------------------------------------------------------------- the three stages
@pytest.mark.parametrize("name", list(VC.CASES))
def test_stft_matches_the_reference(name):
    d = fixture(name)
    net = case_net(name)
    B, Cn, L = d["wav"].shape
    T, Tl_pad, _ = VC.frames_of(name)
    re, im = net._stft(cuda(d["wav"]).reshape(B * Cn, L), net.n_fft // 2 + Tl_pad, T)
    spec = VR._complex(re, im, B, Cn).cpu().numpy()
    assert spec.shape == d["spec"].shape
    peak = np.abs(d["spec"]).max(axis=2, keepdims=True)
    silent = np.broadcast_to(peak == 0, spec.shape)          # frames that lie wholly in the zero padding
    assert not silent.all() and (spec[silent] == 0).all()
    err = np.maximum(np.abs(spec.real - d["spec"].real), np.abs(spec.imag - d["spec"].imag)) / np.where(peak == 0, 1, peak)
    print(f"{name}: stft max|d| / frame peak = {err.max():.2e}")
    assert err.max() <= 1e-5


@pytest.mark.parametrize("name", list(VC.CASES))
def test_mask_matches_the_reference(name):
    d = fixture(name)
    mask = case_net(name)(cuda(d["spec"])).cpu().numpy()
    assert mask.shape == d["mask"].shape and np.isfinite(mask.real).all() and np.isfinite(mask.imag).all()
    dm = float(np.abs(mask - d["mask"]).max())
    sub, ref_sub = mask64_of(name, mask)
    e_ref = float(np.abs(ref_sub - d["mask64"]).max())
    e_hip = float(np.abs(sub - d["mask64"]).max())
    print(f"{name}: mask max|d| = {dm:.2e}, e_ref = {e_ref:.2e} e_hip = {e_hip:.2e}")
    assert dm <= 1e-4
    assert e_hip <= 8 * e_ref + 1e-6
    np.testing.assert_array_equal(mask[:, :, -1], mask[:, :, -2])     # the replicated last bin


@pytest.mark.parametrize("name", list(VC.CASES))
def test_istft_and_the_whole_call_match_the_reference(name):
    d = fixture(name)
    net = case_net(name)
    B, Cn, L = d["wav"].shape
    T, Tl_pad, _ = VC.frames_of(name)
    peak = float(np.abs(d["y"]).max())
    e_ref = float(np.abs(d["y"] - d["y64"]).max())
    # the inverse alone: from the reference's product, and from its factors through the fused multiply
    re, im = VR._planar(cuda(d["spec"] * d["mask"]))
    y1 = net._istft(re, im, None, None, net.n_fft // 2 + Tl_pad, L).reshape(B, Cn, L).cpu().numpy()
    sre, sim = VR._planar(cuda(d["spec"]))
    mre, mim = VR._planar(cuda(d["mask"]))
    y2 = net._istft(sre, sim, mre, mim, net.n_fft // 2 + Tl_pad, L).reshape(B, Cn, L).cpu().numpy()
    y3 = net.predict_from_audio(cuda(d["wav"])).cpu().numpy()
    for tag, y in (("istft", y1), ("istft fused mask", y2), ("predict_from_audio", y3)):
        dy = float(np.abs(y - d["y"]).max())
        e_hip = float(np.abs(y - d["y64"]).max())
        print(f"{name}: {tag}: max|d| / peak = {dy / peak:.2e}, e_ref = {e_ref:.2e} e_hip = {e_hip:.2e}")
    for y in (y1, y2, y3):
        assert float(np.abs(y - d["y"]).max()) <= 1e-5 * peak


def test_spec_round_trip_and_reference_methods():
    """audio2spec / spec2audio (no padding to 32 frames) invert each other; predict and predict_mask slice
    ``offset`` frames off both ends."""
    name = "vr_tiny_stereo"
    d = fixture(name)
    net = case_net(name)
    wav = cuda(d["wav"])
    spec = net.audio2spec(wav)
    L = wav.shape[-1]
    assert spec.shape == (1, 2, 65, L // 32 + 1)
    back = net.spec2audio(spec)
    n = back.shape[-1]
    assert n == (L // 32) * 32
    assert float((back - wav[..., :n]).abs().max()) <= 1e-5 * float(wav.abs().max())
    padded = net.audio2spec(wav, use_pad=True)
    assert padded.shape[-1] == 32
    ref = torch.stft(torch.nn.functional.pad(wav.reshape(2, L).cpu(), (160, 187)), 128, 32, window=torch.hann_window(128),
                     return_complex=True, pad_mode="constant")
    assert float((padded.cpu().reshape(2, 65, 32) - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    net.offset = 8
    try:
        s = cuda(d["spec"])
        m = net(s)
        assert torch.equal(net.predict_mask(s), m[..., 8:-8]) and torch.equal(net.predict(s), (s * m)[..., 8:-8])
    finally:
        net.offset = 64


# ---------------------------------------------------------------- extract_harmonic_aperiodic
@pytest.mark.parametrize("name", ["vr_tiny_mono", "vr_tiny_stereo"])
def test_extract_harmonic_aperiodic(name):
    d = fixture(name)
    net = case_net(name)
    wav = d["wav"][0, 0]
    harmonic, aperiodic = VR.extract_harmonic_aperiodic(wav, net)
    assert harmonic.dtype == np.float32 and harmonic.shape == aperiodic.shape == wav.shape
    x = cuda(wav)[None, None].repeat(1, net.channels, 1)
    y, ap = net.separate(x)
    assert torch.equal(y, net.predict_from_audio(x))
    assert torch.equal(ap, x - y)                      # the fused subtraction is the torch subtraction, bit for bit
    want = y[0].mean(dim=0) if not net.is_mono else y[0, 0]
    np.testing.assert_array_equal(harmonic, want.cpu().numpy())
    np.testing.assert_array_equal(aperiodic, (cuda(wav) - want).cpu().numpy())
    assert np.abs(harmonic).max() > 0.01 and np.abs(aperiodic).max() > 0.01


# ---------------------------------------------------------------- batch independence
@pytest.mark.parametrize("name", ["vr_tiny_mono", "vr_full_b2t64"])
def test_rows_equal_their_single_runs(name):
    d = fixture(name)
    net = case_net(name)
    wav = cuda(d["wav"])
    y, ap = net.separate(wav)
    mask = net(cuda(d["spec"]))
    for b in range(wav.shape[0]):
        y1, ap1 = net.separate(wav[b:b + 1])
        assert torch.equal(y1[0], y[b]) and torch.equal(ap1[0], ap[b]), b
        assert torch.equal(net(cuda(d["spec"][b:b + 1]))[0], mask[b]), b


def test_a_row_does_not_depend_on_its_batch_position():
    """Five rows (every row is a recurrence block of its own): the same utterance at positions 0, 2 and 4."""
    d = fixture("vr_tiny_mono")
    net = case_net("vr_tiny_mono")
    a, b = cuda(d["wav"][0:1]), cuda(d["wav"][1:2])
    y1 = net.separate(a)[0]
    y5 = net.separate(torch.cat([a, b, a, b, a]))[0]
    for pos in (0, 2, 4):
        assert torch.equal(y5[pos], y1[0]), pos


# ---------------------------------------------------------------- lifecycle and arguments
def test_close_returns_the_device_memory_and_a_changed_parameter_repacks():
    L = _lib.lib()
    name = "vr_tiny_mono"
    torch.cuda.synchronize()
    live = L.pd_live_device_bytes()
    net = prodiff_amd.CascadedNet(**VC.model_args(name))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in VC.case_params(name).items()})
    net.cuda()
    wav = cuda(fixture(name)["wav"])
    y = net.predict_from_audio(wav)
    assert torch.equal(y, case_net(name).predict_from_audio(wav))
    assert L.pd_live_device_bytes() > live
    h0 = net.handle().value
    assert net.handle().value == h0
    with torch.no_grad():
        net.out.weight.mul_(0.5)
    y2 = net.predict_from_audio(wav)
    assert not torch.equal(y2, y)
    net.close()
    assert L.pd_live_device_bytes() == live


def test_bad_arguments():
    L = _lib.lib()
    net = case_net("vr_tiny_mono")
    h = net.handle()
    B, T = 1, 32
    nb = 65
    re = torch.zeros(B, T, nb, device="cuda")
    out = torch.empty_like(re)
    need = L.pd_vr_workspace_size(h, B, 0)
    assert need > 0 and L.pd_vr_frames(h, 0) == 32 and L.pd_vr_frames(h, 32 * 31) == 64
    ws = torch.empty(need + 256, dtype=torch.uint8, device="cuda")
    wsp, st = C.c_void_p(ws.data_ptr()), _lib.stream_ptr()
    args = (_lib.fptr(re), _lib.fptr(re), _lib.fptr(out), _lib.fptr(out))
    assert L.pd_vr_mask(h, *args, B, 48, wsp, ws.numel(), st) == 1          # PD_ERR_ARG: T not a multiple of 32
    assert L.pd_vr_mask(h, *args, B, T, wsp, need - 1, st) == 3             # PD_ERR_WORKSPACE
    assert L.pd_vr_mask(h, *args, B, T, wsp, need, st) == 0
    y = torch.empty(B, 31 * 32 + 1, device="cuda")
    assert L.pd_vr_istft(h, _lib.fptr(re), _lib.fptr(re), None, None, None, _lib.fptr(y), None, B, T, 64, 31 * 32 + 1,
                         st) == 1                                           # one sample past the inverse's output
    assert L.pd_vr_istft(h, _lib.fptr(re), _lib.fptr(re), _lib.fptr(re), None, None, _lib.fptr(y), None, B, T, 64, 31 * 32,
                         st) == 1                                           # half a mask
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        net.separate(torch.zeros(1, 2, 700, device="cuda"))


def test_graph_replay_equals_the_eager_call():
    d = fixture("vr_tiny_mono")
    net = case_net("vr_tiny_mono")
    wav = cuda(d["wav"])
    eager = net.predict_from_audio(wav).clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = net.predict_from_audio(wav)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
