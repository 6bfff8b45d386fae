"""GPU tests of the separation's bf16 conv mode (pd_vr_set_option PD_VR_OPT_CONV_DTYPE, CascadedNet.set_compute_dtype)
on the five cases of tests/vr_cases.py and their committed fixtures.

Bars:
  fixture     net(spec) and predict_from_audio(wav) in bf16 against the reference's f32 outputs: y under the project's
              bf16 output bar (tests/bf16_bar.py: rel-L2 <= 1e-2, max-rel <= 2e-2), the mask under rel-L2 <= REL_L2;
              every figure goes out on a BF16ERR line, the aperiodic error relative to the aperiodic peak is printed
  emulation   the native bf16 mask against tests/vr_bf16_emul.py's on the same spectrum.  The two differ in the f32
              summation order and in the bf16 roundings of later inputs that this order flips.  The issue that asked
              for this mode argued the flips to about 1e-7 / 4e-3 of the elements per layer and set
                  rel-L2(native, emulation) <= 0.25 rel-L2(emulation, fixture);
              the first MI355X run measured ratios of 0.265, 0.060, 0.453, 0.584 and 0.597 (tiny_mono, tiny_stereo,
              odd, full_t32, full_b2t64).  The cause is the argument, not the kernel: with nothing changed but its
              convs summed in f32 instead of double, the emulation itself moves by 0.15, 0.15, 0.49, 0.59 and 0.60 of
              its distance to the fixture on the CPU, and two f32 orders (1 and 8 threads) differ by 0.42 of it on the
              full net.  A K-term f32 sum carries about sqrt(K) eps of noise relative to its terms, far more relative
              to the small post-ReLU values; every flip costs a whole bf16 step (sqrt(12) times the rms rounding
              error) and travels through the remaining layers as the roundings do.  Over 12 channel permutations the
              CPU's f32-summed emulation lies 8.3e-4 .. 1.44e-3 (tiny_mono; native 1.41e-3), 4.3e-5 .. 8.2e-4
              (tiny_stereo; 1.79e-4), 9.5e-4 .. 1.21e-3 (odd; 1.00e-3) and 2.45e-3 .. 2.53e-3 (full_t32, 4 draws;
              native 2.56e-3) from the double-summed one: the native mask is one more draw of the same quantity.
              So the bar is that quantity, from the emulation's own error:
                  rel-L2(native, emulation) <= ORDER_FACTOR x order_noise(case),     ORDER_FACTOR = 1.5
              order_noise = the largest of 4 (small nets) or 2 (full nets) seeded draws; 1.5 covers a further draw
              (the 12 draws spread by x1.04 on the full net, x1.28 on odd, x1.75 on tiny_mono around their
              median; tiny_stereo's few flips make its draws discrete, the largest of four stands well above the
              rest).  On the full net the bar is about 0.85 of the bf16 error itself: a defect worth two thirds of the
              rounding error (a truncating conversion, a rounding before the interpolation, a wrong border, tap or
              chunk, each at least that large) does not pass; the ratio to rel-L2(emulation, fixture) is printed.
  the rest    bit-equality (torch.equal): fp32 untouched by a switch there and back, rows, batch position, graph
              replay and ragged rows in bf16; live bytes through the mirror's life
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import prodiff_amd
from prodiff_amd import _lib
from tests import bf16_bar
from tests import vr_bf16_emul as E
from tests import vr_cases as VC
from tests.test_gpu_vr import case_net, cuda, fixture
from tests.test_gpu_vr_ragged import clips, padded

pytestmark = pytest.mark.gpu


def new_net(name):
    net = prodiff_amd.CascadedNet(**VC.model_args(name))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in VC.case_params(name).items()})
    return net.cuda()


@functools.lru_cache(maxsize=None)
def bf16_net(args_items, seed):
    """One bf16 model per (architecture, seed) for this module: the session's shared fp32 nets are never switched."""
    a = dict(args_items)
    net = prodiff_amd.CascadedNet(**a)
    P = VC.synth.synth_vr_params(VC.synth.vr_param_shapes(a["n_fft"], a["nout"], a["nout_lstm"], a["is_mono"]), seed)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
    return net.cuda().set_compute_dtype("bf16")


def case_bf16(name):
    return bf16_net(tuple(sorted(VC.model_args(name).items())), VC.CASES[name][7])


@functools.lru_cache(maxsize=None)
def native_mask(name):
    return case_bf16(name)(cuda(fixture(name)["spec"])).cpu().numpy()


def rel_l2(a, b):
    return float(np.linalg.norm(E.pairs(a) - E.pairs(b)) / np.linalg.norm(E.pairs(b)))


# ---------------------------------------------------------------- 1. against the fixture
@pytest.mark.parametrize("name", list(VC.CASES))
def test_bf16_meets_the_bars_against_the_fixture(name):
    d = fixture(name)
    mask = native_mask(name)
    assert mask.shape == d["mask"].shape and np.isfinite(mask.real).all() and np.isfinite(mask.imag).all()
    rel = rel_l2(mask, d["mask"])
    mx = float(np.abs(mask - d["mask"]).max())
    print(f"BF16ERR vr {name} mask rel-L2={rel:.3e} max|d|={mx:.3e}", flush=True)
    np.testing.assert_array_equal(mask[:, :, -1], mask[:, :, -2])     # the replicated last bin
    wav = cuda(d["wav"])
    y, ap = case_bf16(name).separate(wav)
    assert torch.equal(y, case_bf16(name).predict_from_audio(wav)) and torch.equal(ap, wav - y)
    y, ap = y.cpu().numpy(), ap.cpu().numpy()
    ap_ref = d["wav"] - d["y"]
    e_ap = np.abs(ap - ap_ref)
    print(f"BF16ERR vr {name} aperiodic rel-L2={np.linalg.norm(e_ap) / np.linalg.norm(ap_ref):.3e} "
          f"max-rel={e_ap.max() / np.abs(ap_ref).max():.3e} (|ap| / |y| = "
          f"{np.linalg.norm(ap_ref) / np.linalg.norm(d['y']):.2f})", flush=True)
    bf16_bar.assert_bf16_close(y, d["y"], f"vr {name} y")
    assert rel <= bf16_bar.REL_L2


# ---------------------------------------------------------------- 2. against the emulation
@pytest.mark.parametrize("name", list(VC.CASES))
def test_bf16_mask_is_the_emulated_one_up_to_summation_order(name):
    d = fixture(name)
    emul, _ = E.emulated(name)
    native = native_mask(name)
    r_emul = rel_l2(emul, d["mask"])
    r_nat = rel_l2(native, emul)
    print(f"BF16ERR vr {name} rel-L2(native, emulation)={r_nat:.3e} rel-L2(emulation, fixture)={r_emul:.3e} "
          f"ratio={r_nat / r_emul:.3f} max|native - emulation|={np.abs(native - emul).max():.3e}", flush=True)
    bar = E.ORDER_FACTOR * E.order_noise(name)
    print(f"BF16ERR vr {name} order noise of the emulation={E.order_noise(name):.3e} bar={bar:.3e}", flush=True)
    assert r_emul > 1e-4                       # the emulation does round
    assert r_nat <= bar


# ---------------------------------------------------------------- 3. fp32 untouched
@pytest.mark.parametrize("name", ["vr_tiny_mono", "vr_full_t32"])
def test_fp32_is_bit_equal_after_a_switch_there_and_back(name):
    wav = cuda(fixture(name)["wav"])
    y0, ap0 = case_net(name).separate(wav)                 # a net that never switched
    net = new_net(name)
    try:
        yb, apb = net.set_compute_dtype("bf16").separate(wav)
        h = net.handle().value
        y1, ap1 = net.set_compute_dtype("fp32").separate(wav)
        assert net.handle().value == h                     # a switch flips the mode, it does not rebuild
        assert torch.equal(y1, y0) and torch.equal(ap1, ap0)
        assert not torch.equal(yb, y0) and torch.equal(yb, case_bf16(name).separate(wav)[0])
        assert torch.equal(net.set_compute_dtype("bf16").separate(wav)[0], yb)
    finally:
        net.close()


# ---------------------------------------------------------------- 4. rows, position and graph in bf16
@pytest.mark.parametrize("name", ["vr_tiny_mono", "vr_full_b2t64"])
def test_bf16_rows_equal_their_single_runs(name):
    d = fixture(name)
    net = case_bf16(name)
    wav = cuda(d["wav"])
    y, ap = net.separate(wav)
    mask = net(cuda(d["spec"]))
    for b in range(wav.shape[0]):
        y1, ap1 = net.separate(wav[b:b + 1])
        assert torch.equal(y1[0], y[b]) and torch.equal(ap1[0], ap[b]), b
        assert torch.equal(net(cuda(d["spec"][b:b + 1]))[0], mask[b]), b


def test_a_bf16_row_does_not_depend_on_its_batch_position():
    d = fixture("vr_tiny_mono")
    net = case_bf16("vr_tiny_mono")
    a, b = cuda(d["wav"][0:1]), cuda(d["wav"][1:2])
    y1 = net.separate(a)[0]
    y5 = net.separate(torch.cat([a, b, a, b, a]))[0]
    for pos in (0, 2, 4):
        assert torch.equal(y5[pos], y1[0]), pos


def test_bf16_graph_replay_equals_the_eager_call():
    d = fixture("vr_tiny_mono")
    net = case_bf16("vr_tiny_mono")
    wav = cuda(d["wav"])
    eager = net.predict_from_audio(wav).clone()
    assert not torch.equal(eager, case_net("vr_tiny_mono").predict_from_audio(wav))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = net.predict_from_audio(wav)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


# ---------------------------------------------------------------- 5. ragged in bf16
def test_bf16_ragged_rows_equal_their_single_runs():
    """995 samples at hop 32 are 64 frames alone and sit beside a 96-frame row here; NaN past every length."""
    name, lens = "vr_tiny_mono", (995, 2249)
    net = case_bf16(name)
    assert [t for t, _ in prodiff_amd.vr.row_sizes(lens, net.n_fft, net.hop_length)] == [64, 96]
    wav, ls = padded(name, lens, fill=float("nan"))
    y, ap = net.separate(wav, ls)
    assert not torch.isnan(y).any() and not torch.isnan(ap).any()
    for b, (x, n) in enumerate(zip(clips(name, lens), lens)):
        y1, ap1 = net.separate(cuda(x)[None])
        assert torch.equal(y[b, :, :n], y1[0]) and torch.equal(ap[b, :, :n], ap1[0]), n
        assert float(y[b, :, n:].abs().sum()) == 0.0 and float(ap[b, :, n:].abs().sum()) == 0.0, n
        assert not torch.equal(y1, case_net(name).separate(cuda(x)[None])[0])      # it is the bf16 result


# ---------------------------------------------------------------- 6. lifecycle
def test_bf16_mirror_lives_and_dies_with_the_handle():
    L = _lib.lib()
    name = "vr_tiny_mono"
    torch.cuda.synchronize()
    live = L.pd_live_device_bytes()
    net = new_net(name)
    wav = cuda(fixture(name)["wav"])
    y32 = net.predict_from_audio(wav)
    fp32_bytes = L.pd_live_device_bytes()
    assert fp32_bytes > live
    y = net.set_compute_dtype("bf16").predict_from_audio(wav)
    with_mirror = L.pd_live_device_bytes()
    assert with_mirror > fp32_bytes and not torch.equal(y, y32)
    assert torch.equal(y, case_bf16(name).predict_from_audio(wav))
    net.set_compute_dtype("fp32").predict_from_audio(wav)
    net.set_compute_dtype("bf16").predict_from_audio(wav)
    assert L.pd_live_device_bytes() == with_mirror          # later switches only flip the mode
    # a changed parameter repacks the pool and, the mode being applied to the new handle, its mirror
    with torch.no_grad():
        dict(net.named_parameters())["stg1_low_band_net.0.enc1.conv.0.weight"].mul_(0.5)
    y2 = net.predict_from_audio(wav)
    assert not torch.equal(y2, y) and L.pd_live_device_bytes() == with_mirror
    # through ctypes on the live handle: a bad option or value is PD_ERR_ARG and changes nothing
    h, st = net.handle(), _lib.stream_ptr(wav.device)
    assert L.pd_vr_set_option(h, 1, _lib.PD_DTYPE_BF16, st) == 1
    assert L.pd_vr_set_option(h, -1, _lib.PD_DTYPE_F32, st) == 1
    assert L.pd_vr_set_option(h, _lib.PD_VR_OPT_CONV_DTYPE, 2, st) == 1
    assert L.pd_vr_set_option(h, _lib.PD_VR_OPT_CONV_DTYPE, -1, st) == 1
    assert L.pd_vr_set_option(h, _lib.PD_VR_OPT_CONV_DTYPE, _lib.PD_DTYPE_BF16, st) == 0
    assert torch.equal(net.predict_from_audio(wav), y2)
    net.close()
    assert L.pd_live_device_bytes() == live
