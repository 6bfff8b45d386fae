"""CPU tests of the harmonic-noise separation port: the float64 restatement (tests/vr_ref.py) pinned to the
reference's own float64 run (tests/golden/vr_*.npz), the parameter table, the state-dict loading, the frame and
padding arithmetic, the segment form of the inverse transform and the refused dimensions."""
import numpy as np
import pytest
import torch

import prodiff_amd
from prodiff_amd import _lib, synth
from prodiff_amd import vr as VR
from tests import golden_io
from tests import vr_cases as VC
from tests import vr_ref as R


@pytest.fixture(scope="module")
def fixtures():
    return {name: golden_io.load(name) for name in VC.CASES}


@pytest.mark.parametrize("name", list(VC.CASES))
def test_restatement_matches_the_reference_float64(name, fixtures):
    d = fixtures[name]
    n_fft, hop, _, _, mono, B, L, pseed, iseed = VC.CASES[name]
    assert (int(d["param_seed"]), int(d["input_seed"])) == (pseed, iseed)
    np.testing.assert_array_equal(d["wav"], VC.case_wav(name))
    mask, y = R.predict_from_audio(VC.case_params(name), d["wav"], n_fft, hop)
    assert mask.shape == d["spec"].shape and y.shape == (B, 1 if mono else 2, L)
    m64 = mask if name in VC.SMALL else mask.reshape(-1)[d["mask64_pos"]]
    if name not in VC.SMALL:
        np.testing.assert_array_equal(d["mask64_pos"], VC.subset_positions(name, mask.shape))
    assert np.abs(m64 - d["mask64"]).max() <= 1e-9
    assert np.abs(y - d["y64"]).max() <= 1e-9
    # the float32 run the GPU tests compare against is the same computation
    assert np.abs(d["mask"] - mask).max() <= 1e-5
    assert np.abs(d["y"] - d["y64"]).max() <= 1e-5 * np.abs(d["y64"]).max()
    # neither stem is empty, the mask is not saturated
    assert (np.abs(mask) > 0.999).mean() < 0.01 and np.abs(mask).mean() > 0.05
    assert np.abs(d["wav"] - d["y64"]).max() > 0.05


@pytest.mark.parametrize("name", list(VC.CASES))
def test_param_table_is_the_state_dict(name, fixtures):
    keys = [str(k) for k in fixtures[name]["keys"]]
    assert keys == VC.state_dict_keys(name)
    a = VC.model_args(name)
    shapes = synth.vr_param_shapes(a["n_fft"], a["nout"], a["nout_lstm"], a["is_mono"])
    assert list(shapes) == [k for k in keys if not k.endswith("num_batches_tracked")]
    assert len(shapes) == 582
    net = VR.CascadedNet(**a)
    sd = net.state_dict()
    assert list(sd) == list(shapes) and "window" not in sd
    assert all(tuple(sd[k].shape) == tuple(v) for k, v in shapes.items())
    assert _lib.lib().pd_vr_num_params(_lib.C.byref(net.dims())) == len(net.ordered_params()) == 583


def test_load_state_dict_round_trip_ignores_num_batches_tracked():
    name = "vr_tiny_stereo"
    P = VC.case_params(name)
    sd = {}
    for k in VC.state_dict_keys(name):
        sd[k] = torch.tensor(7) if k.endswith("num_batches_tracked") else torch.from_numpy(P[k])
    net = VR.CascadedNet(**VC.model_args(name))
    res = net.load_state_dict(sd)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in net.state_dict().items():
        np.testing.assert_array_equal(v.numpy(), P[k])
    assert net.window.shape == (128,) and prodiff_amd.CascadedNet is VR.CascadedNet
    with pytest.raises(RuntimeError):
        net.load_state_dict({k: v for k, v in sd.items() if k != "out.weight"})


def test_full_model_conv_count_and_draw_rules():
    shapes = synth.vr_param_shapes(2048, 32, 128, True)
    assert sum(1 for k, s in shapes.items() if len(s) == 4) == 104
    P = synth.synth_vr_params(synth.vr_param_shapes(128, 8, 16, True), 3)
    for k, v in P.items():
        assert v.dtype == np.float32 and np.isfinite(v).all(), k
        if synth.vr_is_bn(k) and k.endswith(("weight", "running_var")):
            assert v.min() >= 0.75 and v.max() <= 1.25, k
    w = P["stg3_full_band_net.aspp.bottleneck.conv.0.weight"]
    assert abs(w.std() * np.sqrt(np.prod(w.shape[1:])) - 1.0) < 0.03


@pytest.mark.parametrize("hop", [32, 512])
def test_frame_and_padding_arithmetic(hop):
    """L around multiples of 32 hop: a frame count that is a multiple of 32 gains a whole extra 32 frames, and the
    zero-padded centred transform has exactly T frames."""
    n_fft = 4 * hop
    for mult in (1, 2, 3):
        for dL in (-hop - 1, -hop, -1, 0, 1, hop - 1, hop):
            L = 32 * hop * mult + dL
            T, Tl_pad, T_pad = VR.padded_frames(L, hop)
            n_frames = L // hop + 1
            assert T % 32 == 0 and T > n_frames and T - n_frames <= 32
            assert (T == n_frames + 32) == (n_frames % 32 == 0)
            assert Tl_pad % hop == 0 and 0 <= Tl_pad <= T_pad - Tl_pad and L + T_pad == (T - 1) * hop
            if hop == 32:
                x = torch.nn.functional.pad(torch.zeros(1, L), (Tl_pad, T_pad - Tl_pad))
                s = torch.stft(x, n_fft, hop, window=torch.hann_window(n_fft), return_complex=True, pad_mode="constant")
                assert s.shape[-1] == T
    lib = _lib.lib()
    assert lib.pd_vr_frames(None, 100) == 0


@pytest.mark.parametrize("n_fft,hop", [(128, 32), (256, 64), (192, 64), (128, 16)])
def test_istft_segment_form_equals_torch_istft(n_fft, hop):
    """The inverse as a product over hop-sized segments (the table pd_vr_create builds) against torch.istft in
    float64, imaginary parts at DC and Nyquist included (irfft ignores them)."""
    g = torch.Generator().manual_seed(n_fft + hop)
    T, nb = 32, n_fft // 2 + 1
    spec = torch.complex(torch.randn(nb, T, generator=g, dtype=torch.float64),
                         torch.randn(nb, T, generator=g, dtype=torch.float64))
    ref = torch.istft(spec[None], n_fft, hop, window=torch.hann_window(n_fft, dtype=torch.float64))[0].numpy()
    assert ref.shape == ((T - 1) * hop,)
    for Tl_pad, L in ((0, (T - 1) * hop), (2 * hop, 5 * hop + 3)):
        y = R.istft_by_segments(spec.numpy().T, n_fft, hop, n_fft // 2 + Tl_pad, L)
        assert np.abs(y - ref[Tl_pad:Tl_pad + L]).max() <= 1e-13


@pytest.mark.parametrize("args", [dict(n_fft=96, hop_length=32), dict(n_fft=2048 + 32, hop_length=32),
                                  dict(n_fft=128, hop_length=8), dict(n_fft=128, hop_length=48),
                                  dict(n_fft=128, hop_length=128), dict(n_fft=128, hop_length=32, nout=6),
                                  dict(n_fft=128, hop_length=32, nout_lstm=15), dict(n_fft=128, hop_length=32, nout_lstm=18),
                                  dict(n_fft=128, hop_length=32, nout_lstm=256)])
def test_unsupported_dims_raise(args):
    with pytest.raises(_lib.HipError):
        VR.CascadedNet(**args)
    a = dict(dict(n_fft=128, hop_length=32, nout=8, nout_lstm=16), **args)
    d = _lib.pd_vr_dims(a["n_fft"], a["hop_length"], a["nout"], a["nout_lstm"], 1)
    lib = _lib.lib()
    assert lib.pd_vr_num_params(_lib.C.byref(d)) == 0
    live = lib.pd_live_device_bytes()
    h = _lib.C.c_void_p(0x5a5a)
    arr = (_lib.C.c_void_p * 583)(*[0x1000 + 64 * i for i in range(583)])
    assert lib.pd_vr_create(_lib.C.byref(d), arr, _lib.PD_DTYPE_F32, None, _lib.C.byref(h)) == 4
    assert h.value == 0x5a5a and lib.pd_live_device_bytes() == live


def test_refused_modes_and_devices():
    with pytest.raises(_lib.HipError):
        VR.CascadedNet(128, 32, 8, 16, is_complex=False)
    d = _lib.pd_vr_dims(128, 32, 8, 16, 1)
    lib = _lib.lib()
    h = _lib.C.c_void_p(0x5a5a)
    arr = (_lib.C.c_void_p * 583)(*[0x1000 + 64 * i for i in range(583)])
    assert lib.pd_vr_create(_lib.C.byref(d), arr, _lib.PD_DTYPE_BF16, None, _lib.C.byref(h)) == 4
    net = VR.CascadedNet(128, 32, 8, 16, is_mono=True)
    with pytest.raises(_lib.HipError):      # parameters on the CPU: there is no CPU fallback
        net.separate(torch.zeros(1, 1, 700))
    for name in ("pd_vr_create", "pd_vr_stft", "pd_vr_mask", "pd_vr_istft", "pd_vr_separate", "pd_vr_frames"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
