"""GPU tests of the native variance curves and k-th harmonic isolation (pd_curves) against the reference's own
outputs (tests/golden/kth_*.npz, curves_*.npz, made by tests/golden/gen_golden_curves.py from
component/binarizer/binarizer_utils.py on the CPU, librosa's two functions restated).

Bars:
  k-th harmonic, resid   max|native - reference f32| <= 1e-5 max|y_ref| (the project's waveform bar, test_gpu_vr.py);
                         e_ref and e_hip against the float64 run are printed; an empty mask gives exact zeros
  every curve            max|native - reference f32| <= 1e-4 (the fp32 parity bar), and
                         e_hip = max|native - f64| <= 8 e_ref + 1e-6, e_ref = max|reference f32 - f64|
                         (test_gpu_rmvpe.py's rule)
Tension is compared on curves_voiced_* alone, where its ratio lies in [0.3, 0.8] on every frame: where E_base is
close to E_full, or both are near zero, fp32 rounding of E^2 moves the ratio by ~1e-3 and the 1e-4 clip turns that
into logit jumps of more than 2.
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
from tests import vr_cases as VC

pytestmark = pytest.mark.gpu


def cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


@functools.lru_cache(maxsize=None)
def fixture(name):
    return golden_io.load(name)


@functools.lru_cache(maxsize=None)
def smoother(k):
    return CV.SinusoidalSmoothingConv1d(k) if k else (lambda x: x)


def kth_batch(name):
    """(wav [B, L], f0 [B, T_f0]) of a kth_* fixture: a shorter f0 padded on the right with its last value, which
    is what the kernel does with it anyway."""
    d = fixture(name)
    rows = range(len(CC.KTH[name][5]))
    n = max(len(d[f"f0{r}"]) for r in rows)
    f0 = np.stack([np.pad(d[f"f0{r}"], (0, n - len(d[f"f0{r}"])), mode="edge") for r in rows])
    return np.stack([d[f"wav{r}"] for r in rows]), f0


# ---------------------------------------------------------------- the k-th harmonic
@pytest.mark.parametrize("name", list(CC.KTH))
def test_kth_harmonic_matches_the_reference(name):
    sr, win, hop, L, ks, dlen, _ = CC.KTH[name]
    d = fixture(name)
    wavs, f0s = kth_batch(name)
    for k in ks:
        batch = prodiff_amd.get_kth_harmonic(k, cuda(wavs), cuda(f0s), hop, win, sr)
        assert batch.is_cuda and batch.shape == wavs.shape
        for r in range(len(dlen)):
            wav, f0 = d[f"wav{r}"], d[f"f0{r}"]
            y_ref, y64 = d[f"y{r}_k{k}"], d[f"y64_{r}_k{k}"]
            y = prodiff_amd.get_kth_harmonic(k, wav, f0, hop, win, sr)                    # the numpy front end
            assert isinstance(y, np.ndarray) and y.dtype == np.float32 and y.shape == wav.shape
            yt, resid = CV._core(sr, win, hop).kth_harmonic(k, cuda(wav), cuda(f0), resid=True)
            np.testing.assert_array_equal(yt.cpu().numpy(), y)
            assert torch.equal(resid, cuda(wav) - yt)             # the fused subtraction is the torch subtraction
            peak = float(np.abs(y_ref).max())
            if peak == 0:
                assert np.abs(y).max() == 0 and np.abs(batch[r].cpu().numpy()).max() == 0     # an empty mask: exact zeros
                continue
            e_ref, e_hip = float(np.abs(y_ref - y64).max()), float(np.abs(y - y64).max())
            dy = float(np.abs(y - y_ref).max())
            print(f"{name} row {r} k {k}: max|d| / peak = {dy / peak:.2e}, e_ref / peak = {e_ref / peak:.2e} "
                  f"e_hip / peak = {e_hip / peak:.2e}")
            assert dy <= 1e-5 * peak
            assert float(np.abs(batch[r].cpu().numpy() - y_ref).max()) <= 1e-5 * peak
            # samples that only frames with an empty mask cover
            first, count = CV.kept_bins(d[f"center{r}_k{k}"][:CC.frames_of(L, hop)], win)
            covered = np.zeros(L + win, bool)
            for t in np.nonzero(count)[0]:
                covered[t * hop:t * hop + win] = True
            assert (y[~covered[win // 2:win // 2 + L]] == 0).all()


def test_an_all_unvoiced_f0_gives_exact_zeros():
    sr, win, hop = CC.VOICED["curves_voiced_small"][:3]
    d = fixture("curves_voiced_small")
    sp = cuda(d["sp"])
    L = sp.shape[0]
    T = CC.frames_of(L, hop)
    f0 = torch.zeros(T, device="cuda")
    y = prodiff_amd.get_kth_harmonic(0, sp, f0, hop, win, sr)
    assert y.is_cuda and float(y.abs().max()) == 0.0
    sm = smoother(5)
    e = CR.get_energy(d["sp"], T + 2, hop, win, "amplitude")
    for domain in CC.TENSION_DOMAINS:
        t = prodiff_amd.get_tension(sp, T + 2, f0, hop, win, sr, sm, domain=domain).cpu().numpy()
        want = CR.smooth(CR.tension_from(e, np.zeros_like(e), domain), 5)
        assert np.abs(t - want).max() <= 1e-4, domain
    raw = prodiff_amd.get_tension(sp, T + 2, f0, hop, win, sr, smoother(0), domain="logit").cpu().numpy()
    hi, lo = np.float32(1 - 1e-4), np.float32(1e-4)
    assert raw[-1] == np.float32(np.log(np.float64(lo) / (1 - np.float64(lo))))       # the zero padding: the clip constant
    assert abs(raw[0] - np.log(np.float64(hi) / (1 - np.float64(hi)))) <= 1e-2         # E / (E + 1e-5) at a loud frame
    ratio = prodiff_amd.get_tension(sp, T + 2, f0, hop, win, sr, smoother(0), domain="ratio").cpu().numpy()
    assert (ratio[-2:] == 0).all() and ratio[:T].min() > 0.99


# ---------------------------------------------------------------- the curves
def check_curve(tag, got, d, key):
    want, w64 = d[key], d[key + "64"]
    assert got.shape == want.shape and got.dtype == np.float32 and np.isfinite(got).all(), tag
    dm = float(np.abs(got - want).max())
    e_ref, e_hip = float(np.abs(want - w64).max()), float(np.abs(got - w64).max())
    print(f"{tag}: max|d| = {dm:.2e}, e_ref = {e_ref:.2e} e_hip = {e_hip:.2e}")
    assert dm <= 1e-4, tag
    assert e_hip <= 8 * e_ref + 1e-6, tag


@pytest.mark.parametrize("front", ["numpy", "tensor"])
@pytest.mark.parametrize("name", list(CC.VOICED))
def test_voiced_curves_match_the_reference(name, front):
    sr, win, hop = CC.VOICED[name][:3]
    d = fixture(name)
    ratio = d[CC.curve_key("tension_ratio", 0, CC.frames_of(len(d["sp"]), hop))]
    assert ratio.min() >= 0.3 and ratio.max() <= 0.8 and CC.edge_distance(d["center"]) >= CC.EDGE_MIN
    to = (lambda x: x) if front == "numpy" else cuda
    back = (lambda x: x) if front == "numpy" else (lambda x: x.cpu().numpy())
    sp, ap, f0 = to(d["sp"]), to(d["ap"]), to(d["f0"])
    base = back(prodiff_amd.get_kth_harmonic(0, sp, f0, hop, win, sr))
    assert np.abs(base - d["base"]).max() <= 1e-5 * np.abs(d["base"]).max()
    for mel_len in CC.mel_lens(len(d["sp"]), hop):
        e = back(prodiff_amd.get_energy(sp, mel_len, hop, win, domain="amplitude"))
        assert np.abs(e - CR.get_energy(d["sp"], mel_len, hop, win, "amplitude")).max() <= 1e-6
        for k in (0,) + CC.SMOOTH_K:
            sm = smoother(k)
            tag = f"{name} {front} k {k} mel_len {mel_len}"
            check_curve(tag + " voicing", back(prodiff_amd.get_voicing(sp, mel_len, hop, win, sm)), d,
                        CC.curve_key("voicing", k, mel_len))
            check_curve(tag + " breath", back(prodiff_amd.get_breath(ap, mel_len, hop, win, sm)), d,
                        CC.curve_key("breath", k, mel_len))
            for domain in CC.TENSION_DOMAINS:
                t = back(prodiff_amd.get_tension(sp, mel_len, f0, hop, win, sr, sm, domain=domain))
                check_curve(f"{tag} tension {domain}", t, d, CC.curve_key("tension_" + domain, k, mel_len))


@pytest.mark.parametrize("front", ["numpy", "tensor"])
def test_gated_curves_match_the_reference(front):
    name = "curves_gate"
    sr, win, hop = CC.GATE[name][:3]
    d = fixture(name)
    to = (lambda x: x) if front == "numpy" else cuda
    back = (lambda x: x) if front == "numpy" else (lambda x: x.cpu().numpy())
    sp, ap = to(d["sp"]), to(d["ap"])
    for mel_len in CC.mel_lens(len(d["sp"]), hop):
        for k in (0,) + CC.SMOOTH_K:
            for pad_mode in ("reflect", "constant"):
                for norm in (True, False):
                    extra = ("" if pad_mode == "reflect" else "_constant") + ("" if norm else "_raw")
                    tag = f"{name} {front} k {k} mel_len {mel_len} {pad_mode} norm {norm}"
                    v = back(prodiff_amd.get_voicing(sp, mel_len, hop, win, smoother(k), norm=norm, pad_mode=pad_mode))
                    b = back(prodiff_amd.get_breath(ap, mel_len, hop, win, smoother(k), norm=norm, pad_mode=pad_mode))
                    check_curve(tag + " voicing", v, d, CC.curve_key("voicing", k, mel_len, extra))
                    check_curve(tag + " breath", b, d, CC.curve_key("breath", k, mel_len, extra))
                    if norm and not k:
                        assert v.max() == 1.0 and b.min() == 0.0      # both ends of the clamp
    with pytest.raises(ValueError):
        prodiff_amd.get_energy(sp, 10, hop, win, domain="x")


def test_a_foreign_smooth_func_sees_the_unsmoothed_curve():
    sr, win, hop = CC.VOICED["curves_voiced_small"][:3]
    d = fixture("curves_voiced_small")
    sp, f0 = cuda(d["sp"]), cuda(d["f0"])
    T = CC.frames_of(len(d["sp"]), hop)
    taps = CV.smoothing_taps(5).cuda()
    seen = []

    def torch_conv(x):
        seen.append(x.shape)
        return torch.nn.functional.conv1d(torch.nn.functional.pad(x[None], (2, 2), mode="replicate"), taps[None, None])[0]

    v = prodiff_amd.get_voicing(sp, T, hop, win, torch_conv)
    t = prodiff_amd.get_tension(sp, T, f0, hop, win, sr, torch_conv)
    assert seen == [(1, T), (1, T)]
    assert float((v - prodiff_amd.get_voicing(sp, T, hop, win, smoother(5))).abs().max()) <= 1e-6
    assert float((t - prodiff_amd.get_tension(sp, T, f0, hop, win, sr, smoother(5))).abs().max()) <= 1e-5
    # the native smoothing alone against the same torch convolution
    x = prodiff_amd.get_energy(sp, T, hop, win)
    assert float((smoother(5)(x[None])[0] - torch_conv(x[None])[0]).abs().max()) <= 1e-5
    x3 = torch.stack([x, x.flip(0)])[:, None]
    assert smoother(10)(x3).shape == (2, 1, T) and torch.equal(smoother(10)(x3)[1, 0], smoother(10)(x.flip(0)))


# ---------------------------------------------------------------- composition and the fused call
def test_tension_equals_its_composition():
    """get_kth_harmonic, get_energy twice, the arithmetic in torch float32, then the native smoothing.  The kernel
    evaluates the arithmetic in double and rounds once, torch rounds after each of its five float32 operations: at
    a ratio in [0.3, 0.8] that is within a few 1e-7 of the ratio, 1e-5 of the dB and logit curves."""
    sr, win, hop = CC.VOICED["curves_voiced_small"][:3]
    d = fixture("curves_voiced_small")
    sp, f0 = cuda(d["sp"]), cuda(d["f0"])
    T = CC.frames_of(len(d["sp"]), hop)
    base = prodiff_amd.get_kth_harmonic(0, sp, f0, hop, win, sr)
    ef = prodiff_amd.get_energy(sp, T, hop, win, domain="amplitude")
    eb = prodiff_amd.get_energy(base, T, hop, win, domain="amplitude")
    ratio = torch.sqrt(torch.clamp(ef ** 2 - eb ** 2, min=0)) / (ef + 1e-5)
    sm = smoother(10)
    got = prodiff_amd.get_tension(sp, T, f0, hop, win, sr, sm, domain="ratio")
    assert float((got - sm(torch.clamp(ratio, 0, 1)[None])[0]).abs().max()) <= 1e-6
    t = torch.clamp(ratio, 1e-4, 1 - 1e-4)
    got = prodiff_amd.get_tension(sp, T, f0, hop, win, sr, sm, domain="logit")
    assert float((got - sm(torch.log(t / (1 - t))[None])[0]).abs().max()) <= 1e-5


@pytest.mark.parametrize("name", list(CC.VOICED))
def test_the_fused_call_equals_the_separate_calls(name):
    sr, win, hop = CC.VOICED[name][:3]
    d = fixture(name)
    sp, ap, f0 = cuda(d["sp"]), cuda(d["ap"]), cuda(d["f0"])
    vc = prodiff_amd.VarianceCurves(sr, win, hop, smooth_width=10.4 * hop / sr)
    assert vc.smooth.kernel_size == 10
    for mel_len in CC.mel_lens(len(d["sp"]), hop):
        out = vc(sp, ap, f0, mel_len, return_base=True)
        assert sorted(out) == ["base_harmonic", "breath", "tension", "voicing"]
        assert torch.equal(out["voicing"], prodiff_amd.get_voicing(sp, mel_len, hop, win, vc.smooth))
        assert torch.equal(out["breath"], prodiff_amd.get_breath(ap, mel_len, hop, win, vc.smooth))
        assert torch.equal(out["tension"], prodiff_amd.get_tension(sp, mel_len, f0, hop, win, sr, vc.smooth))
        assert torch.equal(out["base_harmonic"], prodiff_amd.get_kth_harmonic(0, sp, f0, hop, win, sr))
        check_curve(f"{name} fused tension mel_len {mel_len}", out["tension"].cpu().numpy(), d,
                    CC.curve_key("tension_logit", 10, mel_len))
    as_np = vc(d["sp"], d["ap"], d["f0"], mel_len)
    assert isinstance(as_np["voicing"], np.ndarray) and "base_harmonic" not in as_np
    np.testing.assert_array_equal(as_np["tension"], out["tension"].cpu().numpy())
    vc.close()


def vr_model():
    name = "vr_tiny_mono"
    net = prodiff_amd.CascadedNet(**VC.model_args(name))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in VC.case_params(name).items()})
    return net.cuda(), cuda(fixture(name)["wav"][:, 0])


def test_isolate_parts_and_extract_variance_curves():
    net, wav = vr_model()                      # [2, 1297]
    sr, win, hop = 8000, 256, 64
    T = CC.frames_of(wav.shape[1], hop)
    f0 = torch.linspace(200.0, 260.0, T, device="cuda")[None].repeat(2, 1).contiguous()
    f0[0, 3:6] = 0
    y, ap_want = net.separate(wav[:, None])
    sp, ap = prodiff_amd.isolate_parts(wav, f0, net, hop, win, sr)
    assert torch.equal(sp, y[:, 0]) and torch.equal(ap, ap_want[:, 0])
    rest, ap2, base = prodiff_amd.isolate_parts(wav, f0, net, hop, win, sr, base_harmonic=True)
    want = prodiff_amd.get_kth_harmonic(0, sp, f0, hop, win, sr)
    assert torch.equal(base, want) and torch.equal(rest, sp - want) and torch.equal(ap2, ap)
    assert float(base.abs().max()) > 1e-3
    one = prodiff_amd.isolate_parts(wav[0].cpu().numpy(), f0[0].cpu().numpy(), net, hop, win, sr, base_harmonic=True)
    np.testing.assert_array_equal(one[2], base[0].cpu().numpy())
    vc = prodiff_amd.VarianceCurves(sr, win, hop)
    out = vc.extract_variance_curves(wav, f0, net)
    direct = vc(sp, ap, f0, T)
    assert all(torch.equal(out[k], direct[k]) and out[k].shape == (2, T) for k in direct)
    vc.close()
    net.close()


# ---------------------------------------------------------------- batch independence
def test_rows_equal_their_single_runs_and_do_not_depend_on_their_position():
    name = "kth_small"
    sr, win, hop, L, ks, _, _ = CC.KTH[name]
    wavs, f0s = kth_batch(name)
    a, b, fa, fb = cuda(wavs[0:1]), cuda(wavs[1:2]), cuda(f0s[0:1]), cuda(f0s[1:2])
    vc = prodiff_amd.VarianceCurves(sr, win, hop, smooth_width=5.4 * hop / sr)
    T = CC.frames_of(L, hop)
    singles = [vc(a, b, fa, T + 2, return_base=True), vc(b, a, fb, T + 2, return_base=True)]
    five = vc(torch.cat([a, b, a, b, a]), torch.cat([b, a, b, a, b]), torch.cat([fa, fb, fa, fb, fa]), T + 2,
              return_base=True)
    for key in ("voicing", "breath", "tension", "base_harmonic"):
        for pos in range(5):
            assert torch.equal(five[key][pos], singles[pos % 2][key][0]), (key, pos)
    for k in ks:
        y5 = prodiff_amd.get_kth_harmonic(k, torch.cat([a, b, a]), torch.cat([fa, fb, fa]), hop, win, sr)
        y1 = prodiff_amd.get_kth_harmonic(k, a[0], fa[0], hop, win, sr)
        assert torch.equal(y5[0], y1) and torch.equal(y5[2], y1)
    vc.close()


# ---------------------------------------------------------------- graphs, lifecycle, arguments
def test_graph_replay_equals_the_eager_call():
    sr, win, hop = CC.VOICED["curves_voiced_small"][:3]
    d = fixture("curves_voiced_small")
    sp, ap, f0 = cuda(d["sp"]), cuda(d["ap"]), cuda(d["f0"])
    vc = prodiff_amd.VarianceCurves(sr, win, hop)
    vc.core._ws = _lib.Workspace(per_stream=False)     # sized by the eager call, reused on the capture stream
    T = CC.frames_of(len(d["sp"]), hop)
    eager = {k: v.clone() for k, v in vc(sp, ap, f0, T, return_base=True).items()}
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = vc(sp, ap, f0, T, return_base=True)
    for v in out.values():
        v.zero_()
    g.replay()
    torch.cuda.synchronize()
    for k in eager:
        assert torch.equal(out[k], eager[k]), k
    vc.close()


def test_close_returns_the_device_memory_and_two_handles_coexist():
    L = _lib.lib()
    torch.cuda.synchronize()
    CV.close_all()
    live = L.pd_live_device_bytes()
    d = fixture("curves_voiced_small")
    sp, ap, f0 = cuda(d["sp"]), cuda(d["ap"]), cuda(d["f0"])
    a = prodiff_amd.VarianceCurves(8000, 256, 64)
    b = prodiff_amd.VarianceCurves(8000, 512, 128)
    T = CC.frames_of(len(d["sp"]), 64)
    first = a(sp, ap, f0, T)
    assert L.pd_live_device_bytes() > live
    mid = L.pd_live_device_bytes()
    other = b(sp, ap, f0, T)
    assert L.pd_live_device_bytes() > mid
    again = a(sp, ap, f0, T)
    assert all(torch.equal(first[k], again[k]) for k in first)
    assert not torch.equal(first["tension"], other["tension"])
    b.close()
    assert L.pd_live_device_bytes() == mid
    a.close()
    assert L.pd_live_device_bytes() == live


def test_bad_arguments_return_their_code_without_launching():
    L = _lib.lib()
    core = CV._Core(8000, 256, 64)
    h = core.handle("cuda")
    B, n, T_f0 = 1, 64 * 10, 11
    assert L.pd_curves_frames(h, n) == 11 and L.pd_curves_frames(h, 128) == 0 and L.pd_curves_frames(h, 129) == 3
    need = L.pd_curves_workspace_size(h, B, n, T_f0)
    assert need > 0
    ws = torch.empty(need + 256, dtype=torch.uint8, device="cuda")
    wav, f0 = torch.zeros(B, n, device="cuda"), torch.full((B, T_f0), 200.0, device="cuda")
    y = torch.full_like(wav, 7.0)
    wsp, st = C.c_void_p(ws.data_ptr()), _lib.stream_ptr()
    w, f, yp = _lib.fptr(wav), _lib.fptr(f0), _lib.fptr(y)
    assert L.pd_curves_kth_harmonic(h, w, f, 0, yp, None, B, 128, T_f0, wsp, ws.numel(), st) == 1      # L <= win / 2
    assert b"got 128" in L.pd_last_error()
    assert L.pd_curves_kth_harmonic(h, w, f, 0, yp, None, B, n, T_f0, wsp, need - 1, st) == 3           # PD_ERR_WORKSPACE
    assert L.pd_curves_kth_harmonic(h, w, f, -1, yp, None, B, n, T_f0, wsp, ws.numel(), st) == 1        # k < 0
    assert b"got -1" in L.pd_last_error()
    assert L.pd_curves_kth_harmonic(h, w, f, 0, yp, None, B, n, 0, wsp, ws.numel(), st) == 1            # no f0 frame
    assert L.pd_curves_energy(h, w, 2, 1, 11, None, 0, 0, -96.0, -12.0, yp, B, n, wsp, ws.numel(), st) == 1
    assert L.pd_curves_energy(h, w, 0, 1, 0, None, 0, 0, -96.0, -12.0, yp, B, n, wsp, ws.numel(), st) == 1
    assert L.pd_curves_forward(h, w, None, f, 0, 3, 11, None, 0, 1, -96.0, -12.0, None, None, yp, None, B, n, T_f0, wsp,
                               ws.numel(), st) == 1                                                      # tension domain
    assert L.pd_curves_forward(h, w, None, f, 0, 2, 11, None, 0, 1, -96.0, -12.0, None, yp, yp, None, B, n, T_f0, wsp,
                               ws.numel(), st) == 1                                                      # breath without ap
    torch.cuda.synchronize()
    assert float(y.min()) == 7.0                    # nothing was launched
    assert L.pd_curves_kth_harmonic(h, w, f, 0, yp, None, B, n, T_f0, wsp, need, st) == 0
    torch.cuda.synchronize()
    assert float(y.abs().max()) == 0.0
    with pytest.raises(_lib.HipError, match="128"):
        prodiff_amd.get_kth_harmonic(0, torch.zeros(128, device="cuda"), f0[0], 64, 256, 8000)
    with pytest.raises(_lib.HipError):
        prodiff_amd.get_kth_harmonic(-1, wav[0], f0[0], 64, 256, 8000)
    with pytest.raises(_lib.HipError):
        prodiff_amd.get_kth_harmonic(0, wav[0], f0[0, :0], 64, 256, 8000)
    core.close()
