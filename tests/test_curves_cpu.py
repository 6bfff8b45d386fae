"""CPU tests of the variance-curve port: the restatement (tests/curves_ref.py) pinned to the reference's own runs
(tests/golden/kth_*.npz, curves_*.npz, made by tests/golden/gen_golden_curves.py), the sparse-bin form of the k-th
harmonic against the dense torch.stft -> mask -> torch.istft, the conditions on the inputs, the host-side helpers,
the exports and the refused dimensions.

Bars: the k-th harmonic within 1e-5 of its peak (the project's waveform bar), every curve within 1e-4 (the fp32
parity bar), and 1e-6 where the restatement performs the reference's own float32 operations; the float64 runs
within 1e-9.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import prodiff_amd
from prodiff_amd import _lib
from prodiff_amd import curves as CV
from tests import curves_cases as CC
from tests import curves_ref as CR
from tests import golden_io


@functools.lru_cache(maxsize=None)
def fixture(name):
    return golden_io.load(name)


def kth_rows(name):
    d = fixture(name)
    return [(r, d[f"wav{r}"], d[f"f0{r}"]) for r in range(len(CC.KTH[name][5]))]


# ---------------------------------------------------------------- inputs and conditions
@pytest.mark.parametrize("name", list(CC.KTH))
def test_kth_inputs_and_the_mask_edge_condition(name):
    sr, win, hop, L, ks, dlen, _ = CC.KTH[name]
    wavs, f0s = CC.kth_inputs(name)
    d = fixture(name)
    T = CC.frames_of(L, hop)
    for (r, wav, f0), w2, f2, dl in zip(kth_rows(name), wavs, f0s, dlen):
        assert wav.shape == (L,) and f0.shape == (T + dl,) and wav.dtype == f0.dtype == np.float32
        assert np.abs(wav - w2).max() <= 1e-6 and np.abs(f0 - f2).max() <= 1e-3 * np.abs(f0).max()
        for k in ks:
            c = d[f"center{r}_k{k}"]
            assert CC.edge_distance(c) >= CC.EDGE_MIN
            first, count = CV.kept_bins(c[:T], win)
            _, mask = CR.kth_mask(k, f0, L, hop, win, sr)
            np.testing.assert_array_equal(count, mask[:T].sum(axis=1))
            np.testing.assert_array_equal(first[count > 0], mask[:T].argmax(axis=1)[count > 0])
            assert count.max() <= 8
    if name == "kth_small":
        f0 = d["f00"]
        assert (f0[:2] == 0).all() and (f0[-3:] == 0).all() and (f0[7:11] == 0).all() and (f0 != 0).sum() > 20
    if name == "kth_nyquist":
        T = CC.frames_of(L, hop)
        counts = [CV.kept_bins(d[f"center0_k{k}"][:T], win)[1] for k in ks]
        assert any((c == 0).any() for c in counts) and any(((c > 0) & (c < 7)).any() for c in counts)   # beyond, clipped
        assert all((CV.kept_bins(d[f"center1_k{k}"][:T], win)[1] == 0).all() for k in ks)              # center < 1
        assert all(np.abs(d[f"y1_k{k}"]).max() == 0 for k in ks)
    if name == "kth_full":
        c = CV.kept_bins(d["center0_k0"][:T], win)[1]
        assert c.min() >= 7 and c.max() <= 8


@pytest.mark.parametrize("name", list(CC.VOICED))
def test_voiced_inputs_and_the_tension_ratio_condition(name):
    sr, win, hop, T, _ = CC.VOICED[name]
    d = fixture(name)
    L = len(d["sp"])
    assert L == hop * T + 13 and d["f0"].shape == (T,)
    assert CC.edge_distance(d["center"]) >= CC.EDGE_MIN
    for suffix in ("", "64"):
        ratio = d[CC.curve_key("tension_ratio", 0, CC.frames_of(L, hop), suffix)]
        assert ratio.shape == (CC.frames_of(L, hop),) and ratio.min() >= 0.3 and ratio.max() <= 0.8


def test_gate_input_reaches_both_floors_and_both_clamps():
    sr, win, hop, L, _ = CC.GATE["curves_gate"]
    d = fixture("curves_gate")
    T = CC.frames_of(L, hop)
    v, b = d[CC.curve_key("voicing", 0, T, "_raw")], d[CC.curve_key("breath", 0, T, "_raw")]
    assert v.max() > -12.0 and v.min() == v.max() - np.float32(80.0)        # the top_db floor, above db_max
    assert b.max() < -20.0 and abs(b.min() + 100.0) < 1e-3                  # the amin floor, below db_min
    vn, bn = d[CC.curve_key("voicing", 0, T)], d[CC.curve_key("breath", 0, T)]
    assert vn.max() == 1.0 and bn.min() == 0.0
    assert (d["sp"] == 0).sum() >= L // 3


# ---------------------------------------------------------------- the restatement against the reference
@pytest.mark.parametrize("name", list(CC.KTH))
def test_kth_restatement_matches_the_reference(name):
    sr, win, hop, L, ks, _, _ = CC.KTH[name]
    d = fixture(name)
    for r, wav, f0 in kth_rows(name):
        for k in ks:
            y, y64 = d[f"y{r}_k{k}"], d[f"y64_{r}_k{k}"]
            peak = max(float(np.abs(y64).max()), 1e-30)
            mine = CR.kth_harmonic(k, wav, f0, hop, win, sr)
            mine64 = CR.kth_harmonic(k, wav.astype(np.float64), f0.astype(np.float64), hop, win, sr)
            assert np.abs(mine - y).max() <= 1e-6 * peak and np.abs(mine64 - y64).max() <= 1e-9 * peak
            assert np.abs(y - y64).max() <= 1e-5 * peak
            sparse = CR.kth_harmonic_sparse(k, wav, f0, hop, win, sr)
            assert np.abs(sparse - y).max() <= 1e-5 * peak


@pytest.mark.parametrize("name", ["kth_small", "kth_nyquist", "kth_hop2"])
def test_sparse_form_equals_the_dense_transform_in_float64(name):
    sr, win, hop, L, ks, _, _ = CC.KTH[name]
    for r, wav, f0 in kth_rows(name):
        for k in ks:
            # the float32 f0 decides the mask in both, so that only the transforms differ
            dense = CR.kth_harmonic(k, wav.astype(np.float64), f0, hop, win, sr)
            sparse = CR.kth_harmonic_sparse(k, wav, f0, hop, win, sr)
            assert np.abs(sparse - dense).max() <= 1e-12


@pytest.mark.parametrize("name", list(CC.VOICED) + list(CC.GATE))
def test_curve_restatement_matches_the_reference(name):
    d = fixture(name)
    voiced = name in CC.VOICED
    sr, win, hop = (CC.VOICED if voiced else CC.GATE)[name][:3]
    sp, ap = d["sp"], d["ap"]
    L = len(sp)
    for dtype, suffix, same in ((np.float32, "", 1e-6), (np.float64, "64", 1e-9)):
        s, a = sp.astype(dtype), ap.astype(dtype)
        base = d["base" + suffix] if voiced else None
        for mel_len in CC.mel_lens(L, hop):
            for k in (0,) + CC.SMOOTH_K:
                for pad_mode in ("reflect",) if voiced else ("reflect", "constant"):
                    for norm in (True,) if voiced else (True, False):
                        extra = ("" if pad_mode == "reflect" else "_constant") + ("" if norm else "_raw") + suffix
                        # a dB curve before normalisation spans 100: 1e-6 relative to that
                        bar = same if norm else 100 * same
                        for kind, w in (("voicing", s), ("breath", a)):
                            mine = CR.db_curve(w, mel_len, hop, win, k, norm, pad_mode=pad_mode)
                            want = d[CC.curve_key(kind, k, mel_len, extra)]
                            assert mine.shape == want.shape == (mel_len,) and mine.dtype == want.dtype == dtype
                            assert np.abs(mine - want).max() <= bar, (kind, k, mel_len, extra)
                if voiced:
                    for domain in CC.TENSION_DOMAINS:
                        mine = CR.get_tension(s, mel_len, d["f0"].astype(dtype), hop, win, sr, k, domain=domain, base=base)
                        want = d[CC.curve_key("tension_" + domain, k, mel_len, suffix)]
                        assert np.abs(mine - want).max() <= (100 * same if domain == "db" else 10 * same), (domain, k, mel_len)
    for key in [k for k in d if k.endswith("64") and k[:-2] in d and k != "base64"]:
        assert np.abs(d[key[:-2]] - d[key]).max() <= 1e-4, key


# ---------------------------------------------------------------- host-side helpers
def test_taps_equal_the_reference_bit_for_bit():
    d = fixture("curves_taps")
    for k in CC.TAP_SIZES:
        conv = CV.SinusoidalSmoothingConv1d(k)
        assert conv.weight.shape == (1, 1, k) and conv.weight.dtype == torch.float32
        np.testing.assert_array_equal(conv.weight.numpy().reshape(-1), d[f"taps{k}"])
        np.testing.assert_array_equal(CR.smoothing_taps(k), d[f"taps{k}"])
    assert CV.same_padding(10) == (4, 5) and CV.same_padding(5) == (2, 2) and CV.same_padding(4) == (1, 2)
    for k in (10, 5, 4):
        x = torch.arange(12, dtype=torch.float32) ** 1.5
        conv = torch.nn.Conv1d(1, 1, k, bias=False, padding="same", padding_mode="replicate")
        conv.weight.data = CV.smoothing_taps(k)[None, None]
        assert np.abs(conv(x[None])[0].detach().numpy() - CR.smooth(x.numpy(), k)).max() <= 1e-5


def test_refused_python_arguments():
    for k in (0, 1, 2):
        with pytest.raises(ValueError):
            CV.SinusoidalSmoothingConv1d(k)
    with pytest.raises(ValueError):
        CV.get_energy(np.zeros(1000, np.float32), 10, 64, 256, domain="x")
    with pytest.raises(ValueError):
        CV.VarianceCurves(8000, 256, 64, tension_domain="x")
    with pytest.raises(ValueError):
        CV.VarianceCurves(8000, 256, 64, pad_mode="edge")
    with pytest.raises(_lib.HipError):      # inputs on the CPU: there is no CPU fallback
        CV.get_energy(torch.zeros(1000), 10, 64, 256)
    with pytest.raises(_lib.HipError):
        CV.SinusoidalSmoothingConv1d(5)(torch.zeros(1, 20))
    for args, value in (((8000, 100, 25), "100"), ((8000, 8192, 2048), "8192"), ((8000, 256, 100), "100"),
                        ((8000, 256, 256), "256"), ((8000, 256, 8), "8"), ((8000, 256, 64, 4.0), "4.0"),
                        ((8000, 256, 64, 0.0), "0.0"), ((0, 256, 64), "0")):
        with pytest.raises(_lib.HipError, match=value):
            CV._Core(*args)
    core = CV._Core(8000, 256, 64)
    with pytest.raises(_lib.HipError, match="128"):
        core._rows(torch.zeros(128))
    assert CV.num_frames(64 * 37 + 13, 64) == 38 and CV.num_frames(64 * 37, 64) == 38
    assert production_kernel_size(44100, 512) == 10
    assert prodiff_amd.get_tension is CV.get_tension and prodiff_amd.VarianceCurves is CV.VarianceCurves


def production_kernel_size(sr, hop):
    """The production smoothing kernel: round(0.12 / (hop / sr))."""
    vc = CV.VarianceCurves(sr, 4 * hop, hop)
    return vc.smooth.kernel_size


# ---------------------------------------------------------------- the C-ABI without a device
def test_exports_and_refused_dimensions():
    lib = _lib.lib()
    for name in ("pd_curves_create", "pd_curves_destroy", "pd_curves_frames", "pd_curves_workspace_size",
                 "pd_curves_kth_harmonic", "pd_curves_energy", "pd_curves_smooth", "pd_curves_forward"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.pd_version() == 2
    live = lib.pd_live_device_bytes()
    for dims, value in (((8000, 100, 25, 3.5), b"got 100"), ((8000, 4160, 1040, 3.5), b"got 4160"),
                        ((8000, 32, 16, 3.5), b"got 32"), ((8000, 256, 100, 3.5), b"got 100"),
                        ((8000, 256, 256, 3.5), b"got 256"), ((8000, 256, 8, 3.5), b"got 8"),
                        ((8000, 256, 0, 3.5), b"got 0"), ((8000, 256, 64, 3.75), b"got 3.75"),
                        ((8000, 256, 64, 0.0), b"got 0.0"), ((0, 256, 64, 3.5), b"got 0")):
        h = C.c_void_p(0x5a5a)
        assert lib.pd_curves_create(C.byref(_lib.pd_curves_dims(*dims)), None, C.byref(h)) == 1     # PD_ERR_ARG
        assert value in lib.pd_last_error(), (dims, lib.pd_last_error())
        assert h.value == 0x5a5a and lib.pd_live_device_bytes() == live
    assert lib.pd_curves_create(None, None, None) == 1 and b"null" in lib.pd_last_error()


def test_null_handles_fail_loudly():
    lib = _lib.lib()
    assert lib.pd_curves_frames(None, 4096) == 0 and lib.pd_curves_workspace_size(None, 1, 4096, 10) == 0
    p = C.c_void_p(0x1000)
    assert lib.pd_curves_kth_harmonic(None, p, p, 0, p, None, 1, 4096, 10, p, 1 << 20, None) == 1
    assert b"null" in lib.pd_last_error()
    assert lib.pd_curves_energy(None, p, 0, 1, 10, None, 0, 0, -96.0, -12.0, p, 1, 4096, p, 1 << 20, None) == 1
    assert lib.pd_curves_forward(None, p, p, p, 0, 2, 10, None, 0, 1, -96.0, -12.0, p, p, p, None, 1, 4096, 10, p, 1 << 20,
                                 None) == 1
    assert lib.pd_curves_smooth(None, p, 5, p, 1, 10, None) == 1 and b"null" in lib.pd_last_error()
    assert lib.pd_curves_smooth(p, p, 2, p, 1, 10, None) == 1 and b"got 2" in lib.pd_last_error()
    assert lib.pd_curves_smooth(p, p, 258, p, 1, 10, None) == 1 and b"got 258" in lib.pd_last_error()
    assert lib.pd_curves_smooth(p, p, 5, p, 1, 0, None) == 1 and b"got 0" in lib.pd_last_error()
    lib.pd_curves_destroy(None)
