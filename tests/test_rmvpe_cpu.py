"""CPU tests of the RMVPE port: the float64 restatement (tests/rmvpe_ref.py) pinned to the reference's own
float64 outputs (tests/golden/rmvpe_*.npz), the parameter table, the state-dict loading, the HTK filterbank,
the decode restatement on hand-built salience and the curve helpers of ``get_pitch``."""
import numpy as np
import pytest
import torch

import prodiff_amd
from prodiff_amd import rmvpe as RM
from prodiff_amd import synth
from prodiff_amd.mel import mel_filterbank, mel_filterbank64
from tests import golden_io
from tests import rmvpe_cases as RC
from tests import rmvpe_ref as R


# ---------------------------------------------------------------- restatement and parameter table
@pytest.mark.parametrize("name", list(RC.CASES))
def test_restatement_matches_the_reference_float64(name):
    d = golden_io.load(name)
    model, B, T, pseed, iseed = RC.CASES[name]
    assert (int(d["param_seed"]), int(d["input_seed"])) == (pseed, iseed)
    np.testing.assert_array_equal(d["mel"], RC.case_mel(name))
    feat, hidden = R.e2e0(RC.case_params(name), model, d["mel"])
    assert feat.shape == (B, T, 3 * RC.N_MELS) and hidden.shape == (B, T, RC.N_CLASS)
    assert np.abs(feat - d["feat64"]).max() <= 1e-9
    assert np.abs(hidden - d["hidden64"]).max() <= 1e-9
    # the float32 run the GPU tests compare against is the same computation
    assert np.abs(d["hidden"] - d["hidden64"]).max() <= 1e-5
    assert np.abs(d["feat"] - d["feat64"]).max() <= 1e-5 * np.abs(d["feat64"]).max()


@pytest.mark.parametrize("name", list(RC.CASES))
def test_param_table_is_the_state_dict_without_the_skipped_keys(name):
    keys = [str(k) for k in golden_io.load(name)["keys"]]
    model = RC.CASES[name][0]
    assert list(synth.rmvpe_param_shapes(**model)) == RC.used_keys(keys)
    assert keys == RC.state_dict_keys(model)
    skipped = [k for k in keys if synth.rmvpe_key_is_skipped(k)]
    assert any(k.startswith("unet.tf.") for k in skipped) and any(k.endswith("num_batches_tracked") for k in skipped)


def test_full_model_parameter_count():
    shapes = synth.rmvpe_param_shapes(**RC.FULL)
    stats = sum(int(np.prod(s)) for k, s in shapes.items() if k.endswith(("running_mean", "running_var")))
    # 90 423 165 learnable parameters outside unet.tf, plus the running statistics the fold needs
    assert sum(int(np.prod(s)) for s in shapes.values()) - stats == 90423165


@pytest.mark.parametrize("n_gru", [0, 1])
@pytest.mark.parametrize("en_de_layers", [1, 5])
@pytest.mark.parametrize("n_blocks", [1, 4])
@pytest.mark.parametrize("inter_layers", [1, 4])
def test_num_params_is_the_length_of_the_param_table(n_gru, en_de_layers, n_blocks, inter_layers):
    """pd_rmvpe_num_params counts by running the create walk itself: every branch of that walk (with and without
    the GRU, one level or five, blocks with and without a shortcut, one or several per stage) against the table."""
    from prodiff_amd import _lib
    model = dict(n_blocks=n_blocks, n_gru=n_gru, en_de_layers=en_de_layers, inter_layers=inter_layers,
                 en_out_channels=16)
    dims = _lib.pd_rmvpe_dims(n_blocks, n_gru, en_de_layers, inter_layers, 16, synth.RMVPE_N_MELS,
                              synth.RMVPE_N_CLASS, synth.RMVPE_GRU_HIDDEN)
    assert _lib.lib().pd_rmvpe_num_params(_lib.C.byref(dims)) == len(synth.rmvpe_param_shapes(**model))


def test_draw_rules():
    P = synth.synth_rmvpe_params(synth.rmvpe_param_shapes(**RC.CASES["rmvpe_slim"][0]), 3)
    for k, v in P.items():
        assert v.dtype == np.float32 and np.isfinite(v).all(), k
        if synth._rmvpe_is_bn(k) and k.endswith(("weight", "running_var")):
            assert v.min() >= 0.75 and v.max() <= 1.25, k
        elif synth._rmvpe_is_bn(k) and v.size >= 64:
            assert 0.05 < v.std() < 0.2, k
    w = P["unet.intermediate.layers.0.conv.0.conv.0.weight"]
    assert abs(w.std() * np.sqrt(np.prod(w.shape[1:])) - synth.RMVPE_CONV_GAIN) < 0.02


def test_state_dict_loading_accepts_and_ignores_the_unused_keys():
    model = RC.CASES["rmvpe_shallow"][0]
    net = prodiff_amd.E2E0(model["n_blocks"], model["n_gru"], (2, 2), model["en_de_layers"], model["inter_layers"], 1,
                           model["en_out_channels"])
    assert list(net.state_dict()) == list(synth.rmvpe_param_shapes(**model))
    P = RC.case_params("rmvpe_shallow")
    sd = {}
    for k in RC.state_dict_keys(model):
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.tensor(7)
        elif k.startswith("unet.tf."):
            sd[k] = torch.zeros(3)
        else:
            sd[k] = torch.from_numpy(P[k])
    res = net.load_state_dict(sd, strict=False)          # as component/pe/rmvpe.py:23 calls it
    assert not res.missing_keys and not res.unexpected_keys
    net.load_state_dict(sd)                                # strict
    for k, v in net.state_dict().items():
        np.testing.assert_array_equal(v.numpy(), P[k])
    with pytest.raises(_lib_error()):
        prodiff_amd.E2E0(1, 1, (1, 2))


def _lib_error():
    from prodiff_amd._lib import HipError
    return HipError


# ---------------------------------------------------------------- HTK filterbank
def test_htk_filterbank_properties():
    sr, n_fft, n_mels, fmin, fmax = 16000, 1024, 128, 30, 8000
    fb = mel_filterbank64(sr, n_fft, n_mels, fmin, fmax, htk=True)
    assert fb.shape == (n_mels, n_fft // 2 + 1) and (fb >= 0).all()
    assert np.abs(fb - R.htk_filterbank(sr, n_fft, n_mels, fmin, fmax)).max() <= 1e-12
    assert mel_filterbank(sr, n_fft, n_mels, fmin, fmax, htk=True).dtype == np.float32
    mel = np.linspace(2595 * np.log10(1 + fmin / 700), 2595 * np.log10(1 + fmax / 700), n_mels + 2)
    pts = 700 * (10 ** (mel / 2595) - 1)
    freqs = np.arange(n_fft // 2 + 1) * sr / n_fft
    for m in range(n_mels):
        if fb[m].max() > 0:      # the narrowest low filters may fall between two bins
            assert pts[m] < freqs[fb[m].argmax()] < pts[m + 2], m
    # unit area over Hz: the triangle itself, integrated exactly (height 2 / base, base pts[m + 2] - pts[m])
    height = 2.0 / (pts[2:] - pts[:-2])
    np.testing.assert_allclose(0.5 * height * (pts[2:] - pts[:-2]), 1.0, rtol=0, atol=1e-9)
    for m in range(0, n_mels, 9):
        mid = pts[m + 1]
        j = int(np.searchsorted(freqs, pts[m])), int(np.searchsorted(freqs, pts[m + 2]))
        for k in range(*j):
            tri = min((freqs[k] - pts[m]) / (mid - pts[m]), (pts[m + 2] - freqs[k]) / (pts[m + 2] - mid)) * height[m]
            assert abs(fb[m, k] - tri) <= 1e-9 * height[m]


def test_slaney_filterbank_is_unchanged():
    for args in ((44100, 2048, 128, 40, 16000), (22050, 1024, 80, 20, 11025)):
        a = mel_filterbank(*args)
        b = mel_filterbank(*args, htk=False)
        np.testing.assert_array_equal(a, b)
        assert not np.array_equal(a, mel_filterbank(*args, htk=True))
    with np.load(golden_io.os.path.join(golden_io.GOLDEN, "mel_base.npz")) as z:     # the basis the reference run used
        np.testing.assert_array_equal(z["basis"], mel_filterbank(44100, 2048, 128, 40, 16000))


# ---------------------------------------------------------------- decode restatement
def test_decode_restatement_on_hand_built_salience():
    h = R.decode_cases()
    f0 = R.local_average_f0(h, 0.03)
    cents = 1200 * np.log2(np.where(f0 > 0, f0, 10.0) / 10.0)

    def window(row, lo, hi):
        w = h[row, lo:hi].astype(np.float64)
        return (w * (20.0 * np.arange(lo, hi) + RC.CONST)).sum() / w.sum()

    assert abs(cents[0] - window(0, 0, 5)) < 1e-9           # peak at bin 0: the window is clipped to [0, 5)
    assert abs(cents[1] - window(1, 0, 8)) < 1e-9           # bin 3: [0, 8)
    assert abs(cents[2] - window(2, 352, 360)) < 1e-9       # bin 356: [352, 360)
    assert abs(cents[3] - window(3, 355, 360)) < 1e-9       # bin 359: [355, 360)
    assert f0[4] == 0 and f0[5] == 0                        # all zero; maximum below thred
    assert np.isfinite(R.local_average_f0(h[4], 0.0))       # the sum == 0 guard: no division by zero
    assert R.local_average_f0(h[4], 0.0) == 10.0
    assert h[6, 100] == h[6, 200] == h[6].max()
    assert abs(cents[6] - window(6, 96, 105)) < 1e-9        # a tie: the lowest index
    assert abs(cents[7] - window(7, 180, 189)) < 1e-9
    assert abs(R.local_average_f0(h[7], 0.03, center=np.int64(400)) - 10 * 2 ** (window(7, 355, 360) / 1200)) < 1e-9


def test_decode_restatement_matches_torch():
    h = torch.from_numpy(R.decode_cases())[None].double()
    idx = torch.arange(360, dtype=torch.float64)[None, None, :]      # an int64 idx would round CONST to float32
    center = torch.argmax(h, dim=2, keepdim=True)
    mask = (idx >= torch.clip(center - 4, min=0)) & (idx < torch.clip(center + 5, max=360))
    w = h * mask
    ws = w.sum(2)
    f0 = 10 * 2 ** ((w * (idx * 20 + RC.CONST)).sum(2) / (ws + (ws == 0)) / 1200) * ~(h.max(2)[0] < 0.03)
    np.testing.assert_allclose(R.local_average_f0(h.numpy(), 0.03), f0.numpy(), rtol=1e-12, atol=0)


# ---------------------------------------------------------------- get_pitch's curves
def test_interp_f0():
    f0 = np.array([0.0, 100.0, 0.0, 0.0, 800.0, 0.0])
    out, uv = RM.interp_f0(f0.copy())
    np.testing.assert_array_equal(uv, [True, False, True, True, False, True])
    np.testing.assert_allclose(out, [100.0, 100.0, 200.0, 400.0, 800.0, 800.0], rtol=1e-12)   # linear in log2
    out, uv = RM.interp_f0(np.zeros(4))
    assert uv.all() and (out == 0).all()
    out, uv = RM.interp_f0(np.array([220.0, 330.0]))
    assert not uv.any()
    np.testing.assert_allclose(out, [220.0, 330.0], rtol=1e-12)


def test_resample_align_curve():
    pts = np.array([0.0, 1.0, 2.0, 3.0], np.float32)
    # 10 ms -> 5 ms: t = 0, 5, ..., 25 ms (t_max = 30 ms is excluded)
    out = RM.resample_align_curve(pts, 0.01, 0.005, 6)
    np.testing.assert_allclose(out, [0, 0.5, 1, 1.5, 2, 2.5], atol=1e-6)
    assert out.dtype == np.float32
    np.testing.assert_allclose(RM.resample_align_curve(pts, 0.01, 0.005, 4), [0, 0.5, 1, 1.5], atol=1e-6)           # delta_l < 0
    np.testing.assert_allclose(RM.resample_align_curve(pts, 0.01, 0.005, 8), [0, 0.5, 1, 1.5, 2, 2.5, 2.5, 2.5],
                               atol=1e-6)                                                                          # delta_l > 0
    np.testing.assert_allclose(RM.resample_align_curve(pts, 0.01, 0.02, 3), [0, 2, 2], atol=1e-6)


def test_viterbi_and_uncentred_framing_are_refused():
    with pytest.raises(NotImplementedError):
        RM.RMVPE.decode(None, torch.zeros(1, 1, 360), use_viterbi=True)
    ms = RM.MelSpectrogram(128, 16000, 1024, 160, None, 30, 8000)
    with pytest.raises(NotImplementedError):
        ms.forward_time_major(torch.zeros(1, 2048), center=False)
    assert RM.get_pitch_extractor_cls("rmvpe") is RM.RMVPE
