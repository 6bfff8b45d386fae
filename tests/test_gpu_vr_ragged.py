"""GPU tests of ragged batches through the harmonic-noise separation (pd_vr_separate_ragged and its three stages).

The bar is torch.equal: every row of a ragged batch against that clip run alone through the equal-length entry
point, which tests/test_gpu_vr.py pins to the reference and shows to depend neither on B nor on the row's position.
Once, on the shipped net, the ragged batch also meets the reference fixtures under test_gpu_vr.py's waveform bar.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from prodiff_amd import _lib
from prodiff_amd import vr as VR
from tests import vr_cases as VC
from tests.test_gpu_vr import case_net, cuda, fixture

pytestmark = pytest.mark.gpu

# samples -> frames T_b with hop 32: 995 has 32 real frames, the case where a multiple of 32 gains a whole extra
# block; 7 has one real frame.  Bottom maps of 2, 4 and 6 frames sit under the ASPP's dilations of 2, 4 and 6.
TINY_LENS = (645, 1297, 2249, 995, 7)
TINY_FRAMES = (32, 64, 96, 64, 32)


@functools.lru_cache(maxsize=None)
def clips(name, lens):
    """One [C, L_b] clip per length, every row its own glide and noise (vr_cases.gliding_signal)."""
    n_fft, mono = VC.CASES[name][0], VC.CASES[name][4]
    Cn = 1 if mono else 2
    period = 44100.0 * n_fft / 2048
    return tuple(np.stack([VC.gliding_signal(L, period, 170.0 + 35.0 * (b * Cn + c), 240.0 + 50.0 * (b * Cn + c),
                                             7000 + 10 * b + c) for c in range(Cn)]) for b, L in enumerate(lens))


@functools.lru_cache(maxsize=None)
def singles(name, lens):
    """(harmonic, aperiodic) [C, L_b] of every clip run alone, computed once."""
    net = case_net(name)
    return tuple(tuple(t[0].clone() for t in net.separate(cuda(x)[None])) for x in clips(name, lens))


def padded(name, lens, fill=0.0, order=None):
    xs = clips(name, lens)
    order = list(range(len(lens))) if order is None else order
    out = torch.full((len(lens), xs[0].shape[0], max(lens)), fill, device="cuda")
    for pos, b in enumerate(order):
        out[pos, :, :lens[b]] = cuda(xs[b])
    return out, [lens[b] for b in order]


def check_rows(name, lens, y, ap, order=None):
    order = list(range(len(lens))) if order is None else order
    for pos, b in enumerate(order):
        h1, a1 = singles(name, lens)[b]
        n = lens[b]
        assert torch.equal(y[pos, :, :n], h1), (name, "harmonic", n)
        assert torch.equal(ap[pos, :, :n], a1), (name, "aperiodic", n)
        assert float(y[pos, :, n:].abs().sum()) == 0.0 and float(ap[pos, :, n:].abs().sum()) == 0.0, (name, n)
        assert not torch.isnan(y[pos]).any() and not torch.isnan(ap[pos]).any()


# ---------------------------------------------------------------- the whole call on the tiny nets
@pytest.mark.parametrize("name", ["vr_tiny_mono", "vr_tiny_stereo"])
def test_every_row_equals_its_single_run(name):
    net = case_net(name)
    h = net.handle()
    assert tuple(_lib.lib().pd_vr_frames(h, n) for n in TINY_LENS) == TINY_FRAMES
    assert [t for t, _ in VR.row_sizes(TINY_LENS, net.n_fft, net.hop_length)] == list(TINY_FRAMES)
    wav, lens = padded(name, TINY_LENS)
    y, ap = net.separate(wav, lens)
    check_rows(name, TINY_LENS, y, ap)
    assert float(y[1].abs().max()) > 0.01 and float(ap[1].abs().max()) > 0.01
    assert torch.equal(net.predict_from_audio(wav, lens), y)


@pytest.mark.parametrize("name", ["vr_tiny_mono", "vr_tiny_stereo"])
def test_nan_past_every_length_in_reversed_order(name):
    net = case_net(name)
    order = list(range(len(TINY_LENS)))[::-1]
    wav, lens = padded(name, TINY_LENS, fill=float("nan"), order=order)
    # the workspace past each row's frames holds NaN as well
    net._ws.get(_lib.lib().pd_vr_workspace_size(net.handle(), len(lens), max(lens)), wav.device)
    for buf in net._ws.bufs.values():
        buf[:buf.numel() // 4 * 4].view(torch.float32).fill_(float("nan"))
    y, ap = net.separate(wav, lens)
    check_rows(name, TINY_LENS, y, ap, order)


def test_scalar_load_widths_with_two_lengths():
    name, lens = "vr_odd", (64 * 25 + 3, 64 * 9 + 11)
    net = case_net(name)
    wav, ls = padded(name, lens, fill=float("nan"))
    y, ap = net.separate(wav, ls)
    check_rows(name, lens, y, ap)


# ---------------------------------------------------------------- the shipped net against the fixtures
def test_the_shipped_net_meets_the_reference_and_its_single_runs():
    a, b = fixture("vr_full_t32"), fixture("vr_full_b2t64")
    net = case_net("vr_full_b2t64")
    assert VC.CASES["vr_full_t32"][7] == VC.CASES["vr_full_b2t64"][7]           # one parameter seed, one model
    rows = [a["wav"][0], b["wav"][0], b["wav"][1]]                              # [1, L] each
    refs = [a["y"][0], b["y"][0], b["y"][1]]
    lens = [r.shape[-1] for r in rows]
    assert lens == [10340, 20497, 20497]
    wav = torch.full((3, 1, max(lens)), float("nan"), device="cuda")
    for i, r in enumerate(rows):
        wav[i, :, :lens[i]] = cuda(r)
    y, ap = net.separate(wav, lens)
    for i, (r, ref) in enumerate(zip(rows, refs)):
        n = lens[i]
        got = y[i, :, :n].cpu().numpy()
        peak = float(np.abs(ref).max())
        d = float(np.abs(got - ref).max())
        print(f"row {i} (L = {n}): max|d| / peak = {d / peak:.2e}")
        assert d <= 1e-5 * peak
        y1, ap1 = net.separate(cuda(r)[None])
        assert torch.equal(y[i, :, :n], y1[0]) and torch.equal(ap[i, :, :n], ap1[0]), i
        assert float(y[i, :, n:].abs().sum()) == 0.0 and float(ap[i, :, n:].abs().sum()) == 0.0


# ---------------------------------------------------------------- the three stages
def test_the_stages_equal_their_single_calls():
    name, lens = "vr_tiny_mono", (645, 1297, 2249)
    net = case_net(name)
    frames = [32, 64, 96]
    sizes = VR.row_sizes(lens, net.n_fft, net.hop_length)
    assert [t for t, _ in sizes] == frames
    wav, ls = padded(name, lens, fill=float("nan"))
    rows = wav[:, 0].contiguous()
    T, L = max(frames), max(lens)
    re, im = net._stft(rows, None, T, lens=ls)
    one = []
    for b, (n, (Tb, lead)) in enumerate(zip(lens, sizes)):
        r1, i1 = net._stft(rows[b:b + 1, :n].contiguous(), lead, Tb)
        assert torch.equal(re[b, :Tb], r1[0]) and torch.equal(im[b, :Tb], i1[0]), b
        assert float(re[b, Tb:].abs().sum()) == 0.0
        one.append((r1, i1))
    # the mask: NaN past every row's frames
    re_n, im_n = re.clone(), im.clone()
    for b, Tb in enumerate(frames):
        re_n[b, Tb:] = float("nan")
        im_n[b, Tb:] = float("nan")
    mre, mim = net._mask(re_n, im_n, 3, frames=frames)
    masks = []
    for b, Tb in enumerate(frames):
        m1 = net._mask(one[b][0], one[b][1], 1)
        assert torch.equal(mre[b, :Tb], m1[0][0]) and torch.equal(mim[b, :Tb], m1[1][0]), b
        masks.append(m1)
    # the inverse, with the fused mask and residual
    y, resid = net._istft(re_n, im_n, mre, mim, None, L, wav=rows, lens=ls)
    for b, (n, (Tb, lead)) in enumerate(zip(lens, sizes)):
        y1, r1 = net._istft(one[b][0], one[b][1], masks[b][0], masks[b][1], lead, n, wav=rows[b:b + 1, :n].contiguous())
        assert torch.equal(y[b, :n], y1[0]) and torch.equal(resid[b, :n], r1[0]), b
        assert float(y[b, n:].abs().sum()) == 0.0 and float(resid[b, n:].abs().sum()) == 0.0
    y2 = net._istft(re_n, im_n, None, None, None, L, lens=ls)
    assert not torch.isnan(y2).any()
    assert torch.equal(y2[0, :lens[0]], net._istft(one[0][0], one[0][1], None, None, sizes[0][1], lens[0])[0])


# ---------------------------------------------------------------- the list front end
@pytest.mark.parametrize("name", ["vr_tiny_mono", "vr_tiny_stereo"])
def test_the_list_form_of_extract_harmonic_aperiodic(name):
    net = case_net(name)
    lens = (645, 1297, 995)
    mono = [x[0] for x in clips(name, lens)]
    out = VR.extract_harmonic_aperiodic(mono, net)
    assert isinstance(out, list) and len(out) == 3
    for w, (hm, apd) in zip(mono, out):
        h1, a1 = VR.extract_harmonic_aperiodic(w, net)
        assert hm.dtype == np.float32 and hm.shape == w.shape
        np.testing.assert_array_equal(hm, h1)
        np.testing.assert_array_equal(apd, a1)


# ---------------------------------------------------------------- graph replay
def test_graph_replay_equals_the_eager_call():
    name = "vr_tiny_mono"
    net = case_net(name)
    wav, lens = padded(name, TINY_LENS)
    eager = [t.clone() for t in net.separate(wav, lens)]        # also uploads the sizes: the capture holds no host copy
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = net.separate(wav, lens)
    for t in out:
        t.fill_(7.0)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])


# ---------------------------------------------------------------- arguments
def test_bad_arguments_are_refused_without_launching():
    L = _lib.lib()
    name = "vr_tiny_mono"
    net = case_net(name)
    h = net.handle()
    wav, lens = padded(name, TINY_LENS)
    B, n = wav.shape[0], wav.shape[-1]
    y = torch.full_like(wav, 7.0)
    need = L.pd_vr_workspace_size(h, B, n)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    wsp, st = C.c_void_p(ws.data_ptr()), _lib.stream_ptr()
    ld = torch.tensor(lens, dtype=torch.int32, device="cuda")
    assert L.pd_vr_separate_ragged(h, _lib.fptr(wav), None, _lib.fptr(y), None, B, n, wsp, need, st) == 1      # lens NULL
    assert L.pd_vr_separate_ragged(h, _lib.fptr(wav), _lib.iptr(ld), _lib.fptr(y), None, B, n, wsp, need - 1, st) == 3
    T = L.pd_vr_frames(h, n)
    spec = torch.zeros(B, T, net.output_bin, device="cuda")
    sp = _lib.fptr(spec)
    assert L.pd_vr_mask_ragged(h, sp, sp, None, _lib.fptr(y), _lib.fptr(y), B, T, wsp, need, st) == 1          # frames NULL
    assert L.pd_vr_stft_ragged(h, _lib.fptr(wav), None, sp, sp, B, n, T, st) == 1
    assert L.pd_vr_istft_ragged(h, sp, sp, None, None, None, None, _lib.fptr(y), None, B, T, n, st) == 1
    assert L.pd_vr_istft_ragged(h, sp, sp, None, None, None, _lib.iptr(ld), _lib.fptr(y), None, B, T - 32, n, st) == 1
    torch.cuda.synchronize()
    assert float(y.min()) == 7.0                                 # nothing was launched
    with pytest.raises(_lib.HipError):
        net.separate(wav, lens[:-1])                             # a wrong count
    with pytest.raises(_lib.HipError):
        net.separate(wav, [0] + lens[1:])                        # below the range
    with pytest.raises(_lib.HipError):
        net.separate(wav, [n + 1] + lens[1:])                    # above it
    with pytest.raises(_lib.HipError):
        net.separate(wav, ld)                                    # lens on the device
    re = torch.zeros(2, 64, net.output_bin, device="cuda")
    with pytest.raises(_lib.HipError):
        net._mask(re, re, 2, frames=[48, 64])                    # not a multiple of 32
    with pytest.raises(_lib.HipError):
        net._mask(re, re, 2, frames=[32, 96])                    # more than T
    torch.cuda.synchronize()


def test_out_of_range_sizes_in_a_direct_call_are_clamped():
    """The clamp contract of the C entry point: a length outside [1, L] is clamped into it, so the call returns
    normally and every access stays inside the row; the row clamped to L equals the full-length single run."""
    L = _lib.lib()
    name = "vr_tiny_mono"
    net = case_net(name)
    h = net.handle()
    lens = (645, 1297)
    wav, _ = padded(name, lens)
    n = wav.shape[-1]
    y, ap = torch.full_like(wav, 7.0), torch.full_like(wav, 7.0)
    need = L.pd_vr_workspace_size(h, 2, n)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    ld = torch.tensor([-5, n + 1000], dtype=torch.int32, device="cuda")
    assert L.pd_vr_separate_ragged(h, _lib.fptr(wav), _lib.iptr(ld), _lib.fptr(y), _lib.fptr(ap), 2, n,
                                   C.c_void_p(ws.data_ptr()), need, _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    y1 = net.separate(wav[1:2])[0]
    assert torch.equal(y[1], y1[0])
    assert float(y[0, :, 1:].abs().sum()) == 0.0                 # row 0 ran as one sample
