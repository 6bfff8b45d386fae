#!/usr/bin/env python
"""Time the native variance curves (prodiff_amd.VarianceCurves, pd_curves_forward) and get_kth_harmonic alone with
HIP events: 1 and 8 utterances x 10 s at 44.1 kHz, window 2048, hop 512 (862 frames), smoothing kernel 10.  After a
warm-up, --rounds rounds alternate in one process between the native calls and the same computation written with
torch ops in eager mode on the same GPU (torch.stft, mask, torch.istft, unfold rms, F.conv1d), --calls calls each;
the medians and the spread are over all rounds.  The eager chain gets its f0 already interpolated on the device (the
reference interpolates with numpy on the host; that host trip is left out of its time).  A per-kernel table comes
from pd_profile_*.  Fails without a GPU.  Prints one JSON line per batch size.

    python tools/bench_curves.py [--calls 20] [--rounds 3] [--warmup 3] [--batches 1,8] [--seconds 10]
    python tools/bench_curves.py --ragged N [--calls 20]

--ragged N times the fused ``VarianceCurves`` call on clips of the first N lengths of tests/golden/ds_lengths.json
(frames times the hop, in samples) three ways: (a) one ragged call on the padded batch with ``lens`` and
``f0_lens``, (b) one call per clip (the only way without ragged batches), (c) one equal-length call on the clips
padded to the longest (its results are not those of the clips alone).  (a) is checked bit-equal to (b) first.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import prodiff_amd  # noqa: E402
from prodiff_amd import _lib  # noqa: E402
from prodiff_amd import curves as CV  # noqa: E402
from tests import curves_cases as CC  # noqa: E402

SR, WIN, HOP, HW = 44100, 2048, 512, 3.5


def time_calls(fn, calls):
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def stats(ms):
    ms = np.sort(np.array(ms))
    return dict(median=round(float(np.median(ms)), 4), min=round(float(ms[0]), 4),
                p90=round(float(ms[int(0.9 * (len(ms) - 1))]), 4))


# ---------------------------------------------------------------- the same computation with torch ops
def torch_kth(wav, f0i, window):
    """binarizer_utils.py:159-192 on a batch, f0i [B, T] already interpolated."""
    n = wav.shape[1]
    spec = torch.stft(wav, n_fft=WIN, win_length=WIN, hop_length=HOP, window=window, center=True,
                      return_complex=True).permute(0, 2, 1)
    n_bins = spec.shape[2]
    idx = torch.arange(n_bins, device=wav.device)[None, None].to(f0i)
    center = f0i[:, :, None] * WIN / SR
    start = torch.clip(center - HW, min=0)
    end = torch.clip(center + HW, max=n_bins)
    mask = (center >= 1) & (idx >= start) & (idx < end)
    spec = spec * mask[:, :spec.shape[1]]
    return torch.istft(spec.permute(0, 2, 1), n_fft=WIN, win_length=WIN, hop_length=HOP, window=window, center=True,
                       length=n)


def torch_rms(wav, mel_len):
    x = F.pad(wav[:, None], (WIN // 2, WIN // 2), mode="reflect")[:, 0].unfold(1, WIN, HOP)
    e = torch.sqrt(torch.mean(x * x, dim=2))
    e = F.pad(e, (0, max(mel_len - e.shape[1], 0)))
    return e[:, :mel_len]


def torch_db(e):
    d = 10.0 * torch.log10(torch.clamp(e * e, min=1e-10))
    return torch.maximum(d, d.max(dim=1, keepdim=True)[0] - 80.0)


def torch_smooth(x, taps):
    k = taps.numel()
    xp = F.pad(x[:, None], ((k - 1) // 2, k - 1 - (k - 1) // 2), mode="replicate")
    return F.conv1d(xp, taps[None, None])[:, 0]


def torch_curves(sp, ap, f0i, window, taps, mel_len):
    base = torch_kth(sp, f0i, window)
    ef, eb = torch_rms(sp, mel_len), torch_rms(base, mel_len)
    t = torch.sqrt(torch.clamp(ef * ef - eb * eb, min=0)) / (ef + 1e-5)
    t = torch.clamp(t, 1e-4, 1 - 1e-4)
    tension = torch_smooth(torch.log(t / (1 - t)), taps)

    def norm(v):
        return (torch.clamp(v, -96.0, -12.0) + 96.0) / 84.0

    voicing = norm(torch_smooth(torch_db(ef), taps))
    breath = norm(torch_smooth(torch_db(torch_rms(ap, mel_len)), taps))
    return voicing, breath, tension


def bench_ragged(a):
    dev = torch.device("cuda:0")
    with open(os.path.join(ROOT, "tests", "golden", "ds_lengths.json")) as f:
        ds = json.load(f)
    sr, hop = int(ds["sr"]), int(ds["hop"])
    frames = [int(v) for v in ds["frames"][:a.ragged]]
    if len(frames) < a.ragged:
        raise SystemExit(f"ds_lengths.json holds {len(frames)} lengths")
    lens = [n * hop for n in frames]
    mels = [CV.num_frames(n, HOP) for n in lens]
    vc = prodiff_amd.VarianceCurves(SR, WIN, HOP)
    rng = np.random.default_rng(0)
    f0s = [CC._contour(m, 200.0 + 5.0 * b, rng, SR, HOP) for b, m in enumerate(mels)]
    for f in f0s:
        f[5:9] = 0
    sps = [torch.from_numpy(CC._stack(CC.interp_f0(f.copy()), n, SR, HOP, rng)).to(dev) for f, n in zip(f0s, lens)]
    aps = [torch.from_numpy((0.05 * rng.standard_normal(n)).astype(np.float32)).to(dev) for n in lens]
    f0s = [torch.from_numpy(f).to(dev) for f in f0s]
    sp, ap, f0 = (torch.zeros(len(lens), max(w), device=dev) for w in (lens, lens, mels))
    for b in range(len(lens)):
        sp[b, :lens[b]], ap[b, :lens[b]], f0[b, :mels[b]] = sps[b], aps[b], f0s[b]

    def ragged():
        return vc.core.forward(sp, ap, f0, mels, vc.smooth, lens=lens, f0_lens=mels)[:3]

    def one_by_one():
        return [vc.core.forward(s, p, f, m, vc.smooth)[:3] for s, p, f, m in zip(sps, aps, f0s, mels)]

    def padded_call():
        return vc.core.forward(sp, ap, f0, max(mels), vc.smooth)[:3]

    with torch.no_grad():
        out = ragged()
        same = all(torch.equal(got[b, :m], want) for b, (m, r) in enumerate(zip(mels, one_by_one()))
                   for got, want in zip(out, r))
        line = {"bench": "curves_ragged", "N": len(lens), "seconds": [round(n / sr, 2) for n in lens], "calls": a.calls,
                "device": torch.cuda.get_device_name(0), "lib": _lib.lib().pd_build_config().decode(),
                "ragged_equals_single_calls": bool(same)}
        for key, fn in (("ragged", ragged), ("single_calls", one_by_one), ("padded", padded_call)):
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            line[key + "_ms"] = stats(time_calls(fn, a.calls))
    print(json.dumps(line), flush=True)
    vc.close()


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--ragged", type=int, default=0, metavar="N")
    ap_.add_argument("--calls", type=int, default=20)
    ap_.add_argument("--rounds", type=int, default=3)
    ap_.add_argument("--warmup", type=int, default=3)
    ap_.add_argument("--batches", default="1,8")
    ap_.add_argument("--seconds", type=float, default=10.0)
    a = ap_.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_curves: no GPU found")
    if a.ragged:
        return bench_ragged(a)
    dev = torch.device("cuda:0")
    L = int(round(a.seconds * SR))
    T = CV.num_frames(L, HOP)
    vc = prodiff_amd.VarianceCurves(SR, WIN, HOP)
    window = nuttall_window(dev)
    taps = vc.smooth.taps(dev)
    for B in [int(v) for v in a.batches.split(",")]:
        rng = np.random.default_rng(B)
        f0 = np.stack([CC._contour(T, 200.0 + 25.0 * b, rng, SR, HOP) for b in range(B)])
        f0[:, 5:9] = 0
        sp = np.stack([CC._stack(CC.interp_f0(f0[b].copy()), L, SR, HOP, rng) for b in range(B)])
        apart = (0.05 * rng.standard_normal((B, L))).astype(np.float32)
        f0i = torch.from_numpy(np.stack([CC.interp_f0(f0[b].copy()) for b in range(B)])).to(dev)
        sp, apart, f0 = torch.from_numpy(sp).to(dev), torch.from_numpy(apart).to(dev), torch.from_numpy(f0).to(dev)

        def fused():
            return vc(sp, apart, f0, T)

        def kth():
            return vc.core.kth_harmonic(0, sp, f0)

        def eager():
            return torch_curves(sp, apart, f0i, window, taps, T)

        def eager_kth():
            return torch_kth(sp, f0i, window)

        fns = dict(native_fused=fused, native_kth=kth, torch_fused=eager, torch_kth=eager_kth)
        with torch.no_grad():
            out, ref = fused(), eager()
            diff = {k: float((out[k] - r).abs().max()) for k, r in zip(("voicing", "breath", "tension"), ref)}
            diff["kth_over_peak"] = float((kth() - eager_kth()).abs().max() / eager_kth().abs().max())
            for fn in fns.values():
                for _ in range(a.warmup):
                    fn()
            torch.cuda.synchronize()
            ms = {k: [] for k in fns}
            for _ in range(a.rounds):
                for k, fn in fns.items():
                    ms[k] += time_calls(fn, a.calls)
        line = {"bench": "curves", "B": B, "samples": L, "T": T, "calls": a.calls * a.rounds,
                "device": torch.cuda.get_device_name(0), "lib": _lib.lib().pd_build_config().decode(),
                "max_abs_diff_vs_torch": diff}
        line.update({k + "_ms": stats(v) for k, v in ms.items()})
        n_prof = 3
        _lib.profile_enable(True)
        for _ in range(n_prof):
            fused()
        torch.cuda.synchronize()
        prof = _lib.profile_summary()
        _lib.profile_enable(False)
        line["kernels_ms_per_call"] = {k: [c // n_prof, round(t_ / n_prof, 4)] for k, (c, t_) in sorted(prof.items())}
        print(json.dumps(line), flush=True)
    vc.close()


def nuttall_window(dev):
    phase = torch.arange(WIN, dtype=torch.float32, device=dev) / WIN * 2 * np.pi
    return 0.355768 - 0.487396 * torch.cos(phase) + 0.144232 * torch.cos(2 * phase) - 0.012604 * torch.cos(3 * phase)


if __name__ == "__main__":
    main()
