"""CPU tests of the separation's bf16 conv mode: the emulation (tests/vr_bf16_emul.py) against the reference's own
f32 outputs (tests/golden/vr_*.npz), and the host side of pd_vr_set_option / CascadedNet.set_compute_dtype.

Bars:
  y      the emulated harmonic part against the fixture's f32 y under the project's bf16 output bar
         (tests/bf16_bar.py: rel-L2 <= 1e-2, max-rel <= 2e-2)
  mask   rel-L2 <= REL_L2 over the real and imaginary parts; its largest absolute error has no project bar: it is
         printed per case and held under MASK_MAX_BAR = 2 x the largest value the native mode measured on an MI355X
         over the five cases (tests/vr_bf16_emul.py says why 2)

Measured (emulation on the CPU | native bf16 mode on an MI355X, tests/test_gpu_vr_bf16.py), mask max|d|:
  vr_tiny_mono     7.77e-3 | 7.95e-3
  vr_tiny_stereo   5.14e-3 | 5.14e-3
  vr_odd           6.28e-3 | 5.13e-3
  vr_full_t32      1.97e-2 | 1.70e-2
  vr_full_b2t64    2.79e-2 | 3.04e-2      -> MASK_MAX_GPU = 3.037e-2, MASK_MAX_BAR = 6.07e-2
(the mask itself is bounded by 1 in magnitude; its rel-L2 error is 2.2e-3 .. 5.4e-3 in both columns)
"""
import numpy as np
import pytest
import torch

from prodiff_amd import _lib
from prodiff_amd import vr as VR
from tests import bf16_bar
from tests import golden_io
from tests import vr_bf16_emul as E
from tests import vr_cases as VC


@pytest.mark.parametrize("name", list(VC.CASES))
def test_emulation_meets_the_bars_against_the_fixture(name):
    d = golden_io.load(name)
    mask, y = E.emulated(name)
    assert mask.shape == d["mask"].shape and y.shape == d["y"].shape
    bf16_bar.assert_bf16_close(y, d["y"], f"vr emulation {name} y")
    rel, _ = bf16_bar.bf16_errors(E.pairs(mask), E.pairs(d["mask"]))
    mx = float(np.abs(mask - d["mask"]).max())
    ap = d["wav"] - d["y"]
    rel_ap = float(np.linalg.norm((d["wav"] - y) - ap) / np.linalg.norm(ap))
    print(f"BF16ERR vr emulation {name} mask rel-L2={rel:.3e} max|d|={mx:.3e} (bar {E.MASK_MAX_BAR:.3e}) "
          f"aperiodic rel-L2={rel_ap:.3e}", flush=True)
    assert rel <= bf16_bar.REL_L2
    assert mx <= E.MASK_MAX_BAR
    # bf16 is not a no-op: the emulation differs from the f32 run by more than f32 rounding
    assert rel > 1e-4


def test_folded_weights_are_bf16_values_and_out_is_left_alone():
    P = VC.case_params("vr_tiny_mono")
    w, b = E.folded(P, "stg1_low_band_net.0.enc1")
    assert (w.float().bfloat16().double() == w).all() and (b.float().double() == b).all()
    g = np.asarray(P["stg1_low_band_net.0.enc1.conv.1.weight"], np.float64)
    var = np.asarray(P["stg1_low_band_net.0.enc1.conv.1.running_var"], np.float64)
    exact = np.asarray(P["stg1_low_band_net.0.enc1.conv.0.weight"], np.float64) * (g / np.sqrt(var + 1e-5))[:, None, None, None]
    assert np.abs(w.numpy() - exact).max() <= 2.0 ** -8 * np.abs(exact).max()


def test_set_option_is_exported_and_refuses_a_null_handle():
    lib = _lib.lib()
    assert "pd_vr_set_option" in _lib.EXPORTS and hasattr(lib, "pd_vr_set_option")
    live = lib.pd_live_device_bytes()
    assert lib.pd_vr_set_option(None, _lib.PD_VR_OPT_CONV_DTYPE, _lib.PD_DTYPE_BF16, None) == 1     # PD_ERR_ARG
    assert lib.pd_vr_set_option(None, _lib.PD_VR_OPT_CONV_DTYPE, _lib.PD_DTYPE_F32, None) == 1
    assert lib.pd_live_device_bytes() == live


def test_set_compute_dtype_on_the_module():
    net = VR.CascadedNet(128, 32, 8, 16, is_mono=True)
    assert net.set_compute_dtype("bf16") is net
    assert net.set_compute_dtype("fp32") is net
    for bad in ("fp16", "bfloat16", None):
        with pytest.raises(ValueError):
            net.set_compute_dtype(bad)
    with pytest.raises(_lib.HipError):      # parameters on the CPU: the mode does not bring a CPU fallback
        net.set_compute_dtype("bf16").separate(torch.zeros(1, 1, 700))
