"""CPU tests of the pitch extractor's bf16 modes: the emulation (tests/rmvpe_bf16_emul.py) against the fixtures'
float64 tensors (tests/golden/rmvpe_*.npz, `hidden64` / `feat64`), and the host side of pd_rmvpe_set_option /
E2E0.set_compute_dtype.

Bars: the project's bf16 bar (tests/bf16_bar.py: rel-L2 <= 1e-2, max-rel <= 2e-2) on `hidden` and `feat`.
"""
import numpy as np
import pytest
import torch

import prodiff_amd
from prodiff_amd import _lib
from prodiff_amd import rmvpe as RM
from tests import bf16_bar
from tests import golden_io
from tests import rmvpe_bf16_emul as E
from tests import rmvpe_cases as RC


@pytest.mark.parametrize("name", list(RC.CASES))
def test_emulation_meets_the_bars_against_the_fixture(name):
    d = golden_io.load(name)
    feat, hidden = E.emulated(name)
    assert feat.shape == d["feat64"].shape and hidden.shape == d["hidden64"].shape
    for key, x in (("hidden", hidden), ("feat", feat)):
        bf16_bar.assert_bf16_close(x, d[key + "64"], f"rmvpe emulation {name} {key}")
        assert E.rel_l2(x, d[key + "64"]) > 1e-5          # bf16 is not a no-op: the emulation does round


@pytest.mark.parametrize("name", ["rmvpe_slim", "rmvpe_full_b2t64"])
def test_the_recurrence_alone_meets_the_bars(name):
    d = golden_io.load(name)
    feat, hidden = E.emulated(name, conv=False, gru=True)
    assert np.abs(feat - d["feat64"]).max() <= 1e-9        # the convs are untouched (test_rmvpe_cpu.py's pin)
    bf16_bar.assert_bf16_close(hidden, d["hidden64"], f"rmvpe emulation {name} hidden (recurrence alone)")
    assert E.rel_l2(hidden, d["hidden64"]) > 1e-5


def test_without_a_gru_the_recurrence_option_changes_nothing():
    for conv in (False, True):
        a, b = E.emulated("rmvpe_nogru", conv=conv, gru=True), E.emulated("rmvpe_nogru", conv=conv, gru=False)
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
    d = golden_io.load("rmvpe_nogru")
    assert np.abs(E.emulated("rmvpe_nogru", False, False)[1] - d["hidden64"]).max() <= 1e-9      # no option: rmvpe_ref


def test_folded_weights_are_bf16_values_near_the_exact_fold():
    P = RC.case_params("rmvpe_shallow")
    for conv, bn, tr in (("unet.encoder.layers.1.conv.0.conv.0.weight", "unet.encoder.layers.1.conv.0.conv.1", False),
                         ("unet.decoder.layers.0.conv1.0.weight", "unet.decoder.layers.0.conv1.1", True)):
        w, b = E.folded(P, conv, bn, transposed=tr)
        assert (E._bf16(w) == w).all() and (E._f32(b) == b).all()
        s = P[bn + ".weight"].astype(np.float64) / np.sqrt(P[bn + ".running_var"].astype(np.float64) + 1e-5)
        exact = P[conv].astype(np.float64) * (s[None, :, None, None] if tr else s[:, None, None, None])
        assert np.abs(w - exact).max() <= 2.0 ** -8 * np.abs(exact).max()
        assert np.abs(w - exact).max() > 0


def test_set_option_is_exported_and_refuses_a_null_handle():
    lib = _lib.lib()
    assert "pd_rmvpe_set_option" in _lib.EXPORTS and hasattr(lib, "pd_rmvpe_set_option")
    assert (_lib.PD_RMVPE_OPT_CONV_DTYPE, _lib.PD_RMVPE_OPT_GRU_DTYPE) == (0, 1)
    live = lib.pd_live_device_bytes()
    for opt in (_lib.PD_RMVPE_OPT_CONV_DTYPE, _lib.PD_RMVPE_OPT_GRU_DTYPE):
        assert lib.pd_rmvpe_set_option(None, opt, _lib.PD_DTYPE_BF16, None) == 1     # PD_ERR_ARG
        assert lib.pd_rmvpe_set_option(None, opt, _lib.PD_DTYPE_F32, None) == 1
    assert lib.pd_live_device_bytes() == live


def test_set_compute_dtype_on_the_module():
    model = RC.CASES["rmvpe_shallow"][0]
    net = prodiff_amd.E2E0(model["n_blocks"], model["n_gru"], (2, 2), model["en_de_layers"], model["inter_layers"], 1,
                           model["en_out_channels"])
    assert net.set_compute_dtype("bf16") is net and net._compute_dtype == ("bf16", "bf16")
    assert net.set_compute_dtype("bf16", recurrence="fp32") is net and net._compute_dtype == ("bf16", "fp32")
    assert net.set_compute_dtype("fp32", "bf16") is net and net._compute_dtype == ("fp32", "bf16")
    assert net.set_compute_dtype("fp32") is net and net._compute_dtype == ("fp32", "fp32")
    for bad in ("fp16", "bfloat16", None):
        with pytest.raises(ValueError):
            net.set_compute_dtype(bad)
        with pytest.raises(ValueError):
            net.set_compute_dtype("bf16", recurrence=bad or "half")
    assert net._compute_dtype == ("fp32", "fp32")          # a refused call changes nothing
    with pytest.raises(_lib.HipError):      # parameters on the CPU: the mode does not bring a CPU fallback
        net.set_compute_dtype("bf16")(torch.zeros(1, RM.N_MELS, 32))
