"""GPU tests of ragged batches through the variance curves and the k-th harmonic isolation
(pd_curves_kth_harmonic_ragged, pd_curves_energy_ragged, pd_curves_forward_ragged) and through the whole chain
behind them.

The bar is torch.equal: every row of a ragged batch against that clip's own equal-length call, which
tests/test_gpu_curves.py pins to the reference.  Once, two fixtures of different lengths go through one ragged
voicing and breath call and meet the reference under test_gpu_curves.py's bars.
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
from tests.test_gpu_curves import check_curve, cuda, fixture, smoother
from tests.test_gpu_vr import case_net

pytestmark = pytest.mark.gpu

SR, WIN, HOP = 8000, 256, 64
LENS = (64 * 37 + 13, 64 * 20 + 1, 64 * 9 + 5, 129)        # 129: the shortest the reflect padding allows, 3 frames
FRAMES = tuple(CC.frames_of(n, HOP) for n in LENS)
MEL_LENS = tuple(CC.mel_lens(n, HOP)[b % 3] for b, n in enumerate(LENS))      # T, T - 1, T + 2, T
F0_LENS = tuple(t + d for t, d in zip(FRAMES, (-2, 3, 0, 0)))


@functools.lru_cache(maxsize=None)
def rows():
    """(sp, ap, f0) float32 per row: a harmonic stack on a gliding f0 with unvoiced runs, and a noise."""
    out = []
    for b, (n, tf) in enumerate(zip(LENS, F0_LENS)):
        rng = np.random.default_rng(4100 + b)
        f0 = CC._contour(tf, 210.0 + 30.0 * b, rng, SR, HOP)
        if tf > 12:
            f0[:2] = 0
            f0[7:11] = 0
            f0[-3:] = 0
        sp = CC._stack(CC.interp_f0(f0.copy()), n, SR, HOP, rng, noise=0.02)
        ap = (0.05 * rng.standard_normal(n)).astype(np.float32)
        out.append((sp, ap, f0))
    return tuple(out)


def batch(fill=0.0, order=None):
    """Padded (sp, ap [B, L], f0 [B, T_f0]) with ``fill`` past every length, and the three size lists."""
    order = list(range(len(LENS))) if order is None else order
    sp = torch.full((len(order), max(LENS)), fill, device="cuda")
    ap = torch.full_like(sp, fill)
    f0 = torch.full((len(order), max(F0_LENS)), fill, device="cuda")
    for pos, b in enumerate(order):
        s, a, f = rows()[b]
        sp[pos, :len(s)], ap[pos, :len(a)], f0[pos, :len(f)] = cuda(s), cuda(a), cuda(f)
    pick = lambda v: [v[b] for b in order]   # noqa: E731
    return sp, ap, f0, pick(LENS), pick(MEL_LENS), pick(F0_LENS)


@functools.lru_cache(maxsize=None)
def core():
    return CV._Core(SR, WIN, HOP)


def row_tensors(b):
    return tuple(cuda(x) for x in rows()[b])


def equal_and_zero_past(got, want, n, tag):
    assert torch.equal(got[:n], want), tag
    assert float(got[n:].abs().sum()) == 0.0 and not torch.isnan(got).any(), tag


@pytest.mark.parametrize("fill,reverse", [(0.0, False), (float("nan"), True)])
def test_kth_harmonic_rows_equal_their_single_calls(fill, reverse):
    order = list(range(len(LENS)))[::-1] if reverse else list(range(len(LENS)))
    sp, _, f0, lens, _, f0_lens = batch(fill, order)
    for k in (0, 1):
        y, resid = core().kth_harmonic(k, sp, f0, resid=True, lens=lens, f0_lens=f0_lens)
        assert y.shape == sp.shape
        for pos, b in enumerate(order):
            s, _, f = row_tensors(b)
            y1, r1 = core().kth_harmonic(k, s, f, resid=True)
            equal_and_zero_past(y[pos], y1, LENS[b], ("y", k, b))
            equal_and_zero_past(resid[pos], r1, LENS[b], ("resid", k, b))
        assert float(y[order.index(0)].abs().max()) > 1e-3


@pytest.mark.parametrize("fill,reverse", [(0.0, False), (float("nan"), True)])
def test_energy_rows_equal_their_single_calls(fill, reverse):
    order = list(range(len(LENS)))[::-1] if reverse else list(range(len(LENS)))
    sp, _, _, lens, mels, _ = batch(fill, order)
    for pad_mode in ("reflect", "constant"):
        for domain, k, norm in (("amplitude", 0, False), ("db", 0, False), ("db", 10, True), ("db", 5, True)):
            sm = smoother(k) if k else None
            e = core().energy(sp, mels, domain, sm, norm, pad_mode=pad_mode, lens=lens)
            assert e.shape == (len(order), max(mels))
            for pos, b in enumerate(order):
                e1 = core().energy(row_tensors(b)[0], MEL_LENS[b], domain, sm, norm, pad_mode=pad_mode)
                equal_and_zero_past(e[pos], e1, MEL_LENS[b], (pad_mode, domain, k, b))


@pytest.mark.parametrize("fill,reverse", [(0.0, False), (float("nan"), True)])
def test_fused_rows_equal_their_single_calls(fill, reverse):
    order = list(range(len(LENS)))[::-1] if reverse else list(range(len(LENS)))
    sp, ap, f0, lens, mels, f0_lens = batch(fill, order)
    for k in CC.SMOOTH_K:
        for domain in CC.TENSION_DOMAINS:
            for return_base in (True, False):
                out = core().forward(sp, ap, f0, mels, smoother(k), domain, return_base=return_base, lens=lens,
                                     f0_lens=f0_lens)
                assert (out[3] is None) == (not return_base)
                for pos, b in enumerate(order):
                    s, a, f = row_tensors(b)
                    one = core().forward(s, a, f, MEL_LENS[b], smoother(k), domain, return_base=return_base)
                    for name, got, want in zip(("voicing", "breath", "tension"), out, one):
                        equal_and_zero_past(got[pos], want, MEL_LENS[b], (name, k, domain, b))
                    if return_base:
                        equal_and_zero_past(out[3][pos], one[3], LENS[b], ("base", k, domain, b))
    # get_tension alone, and a pad mode of its own
    t = core().forward(sp, None, f0, mels, None, "ratio", pad_mode="constant", want_curves=False, lens=lens,
                       f0_lens=f0_lens)
    assert t[0] is None and t[1] is None
    for pos, b in enumerate(order):
        s, _, f = row_tensors(b)
        t1 = core().forward(s, None, f, MEL_LENS[b], None, "ratio", pad_mode="constant", want_curves=False)[2]
        equal_and_zero_past(t[2][pos], t1, MEL_LENS[b], ("tension alone", b))


def test_one_ragged_call_meets_the_reference_fixtures():
    """curves_voiced_small (L = 2381) and curves_gate (L = 2368) as one ragged voicing and one ragged breath call,
    under the bars of test_voiced_curves_match_the_reference and test_gated_curves_match_the_reference."""
    dv, dg = fixture("curves_voiced_small"), fixture("curves_gate")
    assert (len(dv["sp"]), len(dg["sp"])) == (2381, 2368)
    for mel_len in CC.mel_lens(len(dv["sp"]), HOP):
        assert mel_len in CC.mel_lens(len(dg["sp"]), HOP)
        for k in (0,) + CC.SMOOTH_K:
            v = prodiff_amd.get_voicing([cuda(dv["sp"]), cuda(dg["sp"])], mel_len, HOP, WIN, smoother(k))
            b = prodiff_amd.get_breath([cuda(dv["ap"]), cuda(dg["ap"])], mel_len, HOP, WIN, smoother(k))
            key_v, key_b = CC.curve_key("voicing", k, mel_len), CC.curve_key("breath", k, mel_len)
            check_curve(f"ragged voiced k {k} mel_len {mel_len} voicing", v[0].cpu().numpy(), dv, key_v)
            check_curve(f"ragged gate k {k} mel_len {mel_len} voicing", v[1].cpu().numpy(), dg, key_v)
            check_curve(f"ragged voiced k {k} mel_len {mel_len} breath", b[0].cpu().numpy(), dv, key_b)
            check_curve(f"ragged gate k {k} mel_len {mel_len} breath", b[1].cpu().numpy(), dg, key_b)


def test_a_foreign_smooth_func_sees_each_row_cut_to_its_mel_len():
    sp, _, _, lens, mels, _ = batch(float("nan"))
    seen = []

    def halve(x):
        seen.append(tuple(x.shape))
        return 0.5 * x

    got = prodiff_amd.get_voicing(sp, mels, HOP, WIN, halve, norm=False, lens=lens)
    assert seen == [(1, m) for m in mels]
    for b, g in enumerate(got):
        want = 0.5 * prodiff_amd.get_voicing(row_tensors(b)[0], MEL_LENS[b], HOP, WIN, lambda x: x, norm=False)
        assert torch.equal(g, want), b


def test_a_full_window_pair_equals_its_single_calls():
    sr, win, hop, n = CC.KTH["kth_full"][:4]
    d = fixture("kth_full")
    wav, f0 = cuda(d["wav0"]), cuda(d["f00"])
    lens = [n, n // 2]
    f0_lens = [len(f0), CC.frames_of(n // 2, hop)]
    sp = torch.full((2, n), float("nan"), device="cuda")
    ff = torch.full((2, len(f0)), float("nan"), device="cuda")
    sp[0], sp[1, :lens[1]], ff[0], ff[1, :f0_lens[1]] = wav, wav[:lens[1]], f0, f0[:f0_lens[1]]
    ap = 0.5 * sp
    c = CV._Core(sr, win, hop)
    out = c.forward(sp, ap, ff, None, smoother(10), "logit", return_base=True, lens=lens, f0_lens=f0_lens)
    for b in range(2):
        one = c.forward(sp[b, :lens[b]].contiguous(), ap[b, :lens[b]].contiguous(), ff[b, :f0_lens[b]].contiguous(),
                        CC.frames_of(lens[b], hop), smoother(10), "logit", return_base=True)
        for name, got, want, m in zip(("voicing", "breath", "tension", "base"), out, one,
                                      [CC.frames_of(lens[b], hop)] * 3 + [lens[b]]):
            equal_and_zero_past(got[b], want, m, (name, b))
    assert float(out[3][1].abs().max()) > 1e-3
    c.close()


# ---------------------------------------------------------------- the chain
def test_the_chain_on_a_list_of_clips_equals_the_single_calls():
    net = case_net("vr_tiny_mono")
    lens = (1297, 645, 995)
    period = 44100.0 * 128 / 2048
    from tests import vr_cases as VC
    clips = [VC.gliding_signal(n, period, 180.0 + 40.0 * b, 250.0 + 60.0 * b, 8800 + b) for b, n in enumerate(lens)]
    f0s = [np.linspace(200.0, 260.0 + 10 * b, CC.frames_of(n, HOP) + (b - 1)).astype(np.float32) for b, n in enumerate(lens)]
    for f in f0s:
        f[3:6] = 0
    got = prodiff_amd.isolate_parts(clips, f0s, net, HOP, WIN, SR, base_harmonic=True)
    parts = prodiff_amd.isolate_parts(clips, f0s, net, HOP, WIN, SR)
    vc = prodiff_amd.VarianceCurves(SR, WIN, HOP)
    curves = vc.extract_variance_curves(clips, f0s, net, return_base=True)
    for b, (w, f) in enumerate(zip(clips, f0s)):
        one = prodiff_amd.isolate_parts(w, f, net, HOP, WIN, SR, base_harmonic=True)
        for i in range(3):
            assert isinstance(got[i][b], np.ndarray) and got[i][b].shape == w.shape
            np.testing.assert_array_equal(got[i][b], one[i])
        sp1, ap1 = prodiff_amd.isolate_parts(w, f, net, HOP, WIN, SR)
        np.testing.assert_array_equal(parts[0][b], sp1)
        np.testing.assert_array_equal(parts[1][b], ap1)
        c1 = vc.extract_variance_curves(w, f, net, return_base=True)
        assert sorted(curves) == sorted(c1)
        for key in c1:
            np.testing.assert_array_equal(curves[key][b], c1[key])
        assert curves["voicing"][b].shape == (CC.frames_of(len(w), HOP),)
    # padded tensors with lens and f0_lens, and a mel_len per row
    L, Tf = max(lens), max(len(f) for f in f0s)
    wav = torch.full((3, L), float("nan"), device="cuda")
    ff = torch.full((3, Tf), float("nan"), device="cuda")
    for b in range(3):
        wav[b, :lens[b]], ff[b, :len(f0s[b])] = cuda(clips[b]), cuda(f0s[b])
    mels = [CC.frames_of(n, HOP) + 2 - b for b, n in enumerate(lens)]
    out = vc.extract_variance_curves(wav, ff, net, mel_len=mels, lens=list(lens), f0_lens=[len(f) for f in f0s])
    for b in range(3):
        c1 = vc.extract_variance_curves(cuda(clips[b]), cuda(f0s[b]), net, mel_len=mels[b])
        for key in c1:
            assert torch.equal(out[key][b], c1[key]), (key, b)
    vc.close()


# ---------------------------------------------------------------- graph replay
def test_graph_replay_equals_the_eager_call():
    sp, ap, f0, lens, mels, f0_lens = batch()
    c = CV._Core(SR, WIN, HOP)
    c._ws = _lib.Workspace(per_stream=False)       # sized by the eager call, reused on the capture stream
    sm = smoother(10)
    run = lambda: c.forward(sp, ap, f0, mels, sm, "logit", return_base=True, lens=lens, f0_lens=f0_lens)   # noqa: E731
    eager = [t.clone() for t in run()]             # also uploads the sizes: the capture holds no host copy
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = run()
    for t in out:
        t.fill_(7.0)
    g.replay()
    torch.cuda.synchronize()
    for got, want in zip(out, eager):
        assert torch.equal(got, want)
    c.close()


# ---------------------------------------------------------------- arguments
def test_bad_arguments_are_refused_without_launching():
    L = _lib.lib()
    sp, ap, f0, lens, mels, f0_lens = batch()
    c = core()
    h = c.handle("cuda")
    B, n, Tf = sp.shape[0], sp.shape[1], f0.shape[1]
    need = L.pd_curves_workspace_size(h, B, n, Tf)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    wsp, st = C.c_void_p(ws.data_ptr()), _lib.stream_ptr()
    y = torch.full_like(sp, 7.0)
    w, f, yp = _lib.fptr(sp), _lib.fptr(f0), _lib.fptr(y)
    assert L.pd_curves_kth_harmonic_ragged(h, w, f, 0, yp, None, None, B, n, Tf, wsp, need, st) == 1         # rows NULL
    assert L.pd_curves_energy_ragged(h, w, 0, 1, 11, None, 0, 0, -96.0, -12.0, yp, None, B, n, wsp, need, st) == 1
    assert L.pd_curves_forward_ragged(h, w, None, f, 0, 2, 11, None, 0, 1, -96.0, -12.0, None, None, yp, None, None, B, n,
                                      Tf, wsp, need, st) == 1
    rd = torch.tensor([v for t in zip(lens, mels, f0_lens) for v in t], dtype=torch.int32, device="cuda")
    assert L.pd_curves_kth_harmonic_ragged(h, w, f, 0, yp, None, _lib.iptr(rd), B, n, Tf, wsp, need - 1, st) == 3
    torch.cuda.synchronize()
    assert float(y.min()) == 7.0                                   # nothing was launched
    with pytest.raises(_lib.HipError, match="row 3"):
        c.kth_harmonic(0, sp, f0, lens=lens[:3] + [128], f0_lens=f0_lens)       # L_b <= win / 2
    with pytest.raises(_lib.HipError):
        c.kth_harmonic(0, sp, f0, lens=lens[:3], f0_lens=f0_lens)               # a wrong count
    with pytest.raises(_lib.HipError):
        c.kth_harmonic(0, sp, f0, lens=lens[:3] + [n + 1], f0_lens=f0_lens)     # past the row stride
    with pytest.raises(_lib.HipError):
        c.kth_harmonic(0, sp, f0, lens=lens, f0_lens=[0] + f0_lens[1:])
    with pytest.raises(_lib.HipError):
        c.energy(sp, [0] + mels[1:], lens=lens)
    with pytest.raises(_lib.HipError):
        c.forward(sp, ap, f0, mels, lens=torch.tensor(lens, device="cuda"), f0_lens=f0_lens)    # lens on the device
    torch.cuda.synchronize()


def test_out_of_range_sizes_in_a_direct_call_are_clamped():
    """The clamp contract of the C entry points: sizes outside their ranges are clamped into them, so the call
    returns normally and every access stays inside the row; the row clamped to the strides equals the
    full-length single call."""
    L = _lib.lib()
    sp, ap, f0, _, _, _ = batch()
    c = core()
    h = c.handle("cuda")
    B, n, Tf = 2, sp.shape[1], f0.shape[1]
    s2, a2, f2 = sp[:2].contiguous(), ap[:2].contiguous(), f0[:2].contiguous()
    mel = 40
    need = L.pd_curves_workspace_size(h, B, n, Tf)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    rd = torch.tensor([-7, -1, 0, n + 999, mel + 999, Tf + 999], dtype=torch.int32, device="cuda")
    outs = [torch.full((B, mel), 7.0, device="cuda") for _ in range(3)]
    base = torch.full_like(s2, 7.0)
    taps = smoother(5).taps("cuda")
    assert L.pd_curves_forward_ragged(h, _lib.fptr(s2), _lib.fptr(a2), _lib.fptr(f2), 0, 2, mel, _lib.fptr(taps), 5, 1,
                                      -96.0, -12.0, _lib.fptr(outs[0]), _lib.fptr(outs[1]), _lib.fptr(outs[2]),
                                      _lib.fptr(base), _lib.iptr(rd), B, n, Tf, C.c_void_p(ws.data_ptr()), need,
                                      _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    one = c.forward(s2[1], a2[1], f2[1], mel, smoother(5), "logit", return_base=True)
    for got, want in zip(outs + [base], one):
        assert torch.equal(got[1], want)
    assert float(base[0, WIN // 2 + 1:].abs().sum()) == 0.0        # row 0 ran as win / 2 + 1 samples
    assert float(outs[0][0, 1:].abs().sum()) == 0.0                # and one curve frame
