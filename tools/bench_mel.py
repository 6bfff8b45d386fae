#!/usr/bin/env python
"""Time the native mel analysis (prodiff_amd.STFT.get_mel_time_major, one mel_forward_kernel launch) with HIP
events: warm-up, then the median over --calls single calls, at the C5 shape (8 utterances x 861 frames x 512
samples, SVS settings) and at B = 1.  Beside it the same analysis written with torch ops (reflect pad,
torch.stft, abs, matmul, log: what nvSTFT.py:77-96 runs) on the same GPU, when that torch build's stft
works on the device.  Prints one JSON line per shape.

    python tools/bench_mel.py [--calls 100] [--warmup 10] [--keyshift 0] [--speed 1]

The floor: frames x 2 (re, im) x 2 nf nb FLOP on the f32 MFMA (157.3 TFLOP/s dense), plus the mel GEMM.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from prodiff_amd import STFT, _lib  # noqa: E402
from prodiff_amd.mel import derived_sizes  # noqa: E402

F32_MFMA_PEAK = 157.3e12
SVS = dict(sr=44100, n_mels=128, n_fft=2048, win_size=2048, hop_length=512, fmin=40, fmax=16000)


def time_calls(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms = np.sort(np.array(ms))
    return float(np.median(ms)), float(ms[0]), float(ms[int(0.9 * (len(ms) - 1))])


def torch_get_mel(y, basis, window, nf, wn, hn, n_fft, win_size, keyshift, clip):
    yp = torch.nn.functional.pad(y[:, None], ((wn - hn) // 2, (wn - hn + 1) // 2), mode="reflect")[:, 0]
    spec = torch.stft(yp, nf, hop_length=hn, win_length=wn, window=window, center=False, normalized=False,
                      onesided=True, return_complex=True).abs()
    if keyshift != 0:
        size = n_fft // 2 + 1
        if spec.size(1) < size:
            spec = torch.nn.functional.pad(spec, (0, 0, 0, size - spec.size(1)))
        spec = spec[:, :size] * win_size / wn
    return torch.log(torch.clamp(torch.matmul(basis, spec), min=clip))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--frames", type=int, default=861)
    ap.add_argument("--keyshift", type=float, default=0)
    ap.add_argument("--speed", type=float, default=1)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    assert a.calls >= 50, "median over at least 50 calls"
    dev = torch.device("cuda:0")
    s = STFT(**SVS)
    nf, wn, hn = derived_sizes(SVS["n_fft"], SVS["win_size"], SVS["hop_length"], a.keyshift, a.speed)
    nb = min(SVS["n_fft"] // 2 + 1, nf // 2 + 1)
    g = torch.Generator().manual_seed(0)
    for B in (8, 1):
        L = a.frames * SVS["hop_length"]
        y = (torch.rand(B, L, generator=g) * 2 - 1).to(dev)
        out = s.get_mel_time_major(y, a.keyshift, a.speed)
        T = out.shape[1]
        med, best, p90 = time_calls(lambda: s.get_mel_time_major(y, a.keyshift, a.speed), a.calls, a.warmup)
        flop = B * T * (2 * 2 * nf * nb + 2 * nb * SVS["n_mels"])
        tiles = B * ((T + 31) // 32)
        line = {"bench": "mel", "B": B, "frames": T, "samples": L, "keyshift": a.keyshift, "speed": a.speed,
                "nf": nf, "hop": hn, "bins": nb, "calls": a.calls, "native_ms_median": round(med, 4),
                "native_ms_min": round(best, 4), "native_ms_p90": round(p90, 4), "gflop": round(flop / 1e9, 2),
                "f32_mfma_peak_fraction": round(flop / (med * 1e-3) / F32_MFMA_PEAK, 4),
                "floor_ms_at_peak": round(flop / F32_MFMA_PEAK * 1e3, 4), "blocks": tiles,
                "table_bytes_streamed": tiles * 2 * ((nf + 31) // 32 * 32) * ((nb + 31) // 32 * 32) * 4,
                "device": torch.cuda.get_device_name(0), "lib": _lib.lib().pd_build_config().decode()}
        if not a.no_torch:
            try:
                basis = s.mel_basis_host.to(dev)
                window = torch.hann_window(wn, device=dev)
                args = (y, basis, window, nf, wn, hn, SVS["n_fft"], SVS["win_size"], a.keyshift, s.clip_val)
                ref = torch_get_mel(*args)
                line["torch_max_abs_diff"] = float((ref.transpose(1, 2) - out).abs().max())
                tm, tb, _ = time_calls(lambda: torch_get_mel(*args), a.calls, a.warmup)
                line["torch_ms_median"], line["torch_ms_min"] = round(tm, 4), round(tb, 4)
            except Exception as e:   # torch.stft on this build / device
                line["torch_error"] = f"{type(e).__name__}: {e}"[:300]
        print(json.dumps(line), flush=True)
    s.close()


if __name__ == "__main__":
    main()
