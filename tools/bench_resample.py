#!/usr/bin/env python
"""Time the native sample-rate conversion (prodiff_amd.Resample, one resample_forward_kernel launch) with HIP
events: warm-up, then the median over --calls single calls, at 8 utterances x 10 s, 48 -> 44.1 kHz with
KAISER_BEST and 44.1 -> 16 kHz with the Hann window at lowpass_filter_width 128 (the RMVPE front end).  Beside
each the same table through torch.nn.functional.conv1d(stride=o) on the same GPU: padding (W, W + o), conv,
truncation, which is what torchaudio.functional.resample runs.  Also the kernel alone (the library's event pair
around the launch) and the per-call time of 20 calls replayed back to back from one hipGraph.  Prints one JSON
line per shape.

    python tools/bench_resample.py [--calls 100] [--warmup 10] [--seconds 10] [--batch 8]

The floors: 2 K FLOP per output sample on the f32 MFMA (157.3 TFLOP/s dense); 4 bytes read per input sample and
4 written per output sample over HBM (8 TB/s).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from prodiff_amd import KAISER_BEST, Resample, _lib  # noqa: E402

F32_MFMA_PEAK = 157.3e12
HBM_PEAK = 8.0e12
GRAPH_CALLS = 20
SHAPES = [("48k_to_44k1_kaiser_best", 48000, 44100, KAISER_BEST),
          ("44k1_to_16k_hann128", 44100, 16000, dict(resampling_method="sinc_interp_hann", lowpass_filter_width=128))]


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


def torch_resample(y, kernel, W, o, n, target):
    yp = torch.nn.functional.pad(y[:, None], (W, W + o))
    out = torch.nn.functional.conv1d(yp, kernel[:, None], stride=o)          # [B, n, Q]
    return out.transpose(1, 2).reshape(y.shape[0], -1)[:, :target]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    assert a.calls >= 50, "median over at least 50 calls"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    for name, orig, new, kw in SHAPES:
        r = Resample(orig, new, **kw)
        B, L = a.batch, int(round(a.seconds * orig))
        y = (torch.rand(B, L, generator=g) * 2 - 1).to(dev)
        out = r(y)
        M, K = out.shape[1], 2 * r.width + r.o
        med, best, p90 = time_calls(lambda: r(y), a.calls, a.warmup)
        # the kernel alone (the library's own event pair around the launch): a call also holds the Python layer
        _lib.profile_filter(["resample_forward"])
        _lib.profile_enable(True)
        for _ in range(a.calls):
            r(y)
        torch.cuda.synchronize()
        cnt, total = _lib.profile_summary()["resample_forward"]
        _lib.profile_enable(False)
        kern = total / cnt
        # back to back: GRAPH_CALLS calls captured into one hipGraph (the call allocates nothing but its output),
        # per-call time of a replay -- the kernel under sustained load, without the host between launches
        graph_ms = graph_error = None
        try:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                r(y)
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for _ in range(GRAPH_CALLS):
                    r(y)
            graph_ms = time_calls(graph.replay, 50, 5)[0] / GRAPH_CALLS
            del graph
        except Exception as e:   # capture on this build / device
            graph_error = f"{type(e).__name__}: {e}"[:300]
        flop = 2.0 * K * B * M
        nbytes = 4.0 * B * (L + M)
        floor_ms = max(flop / F32_MFMA_PEAK, nbytes / HBM_PEAK) * 1e3
        line = {"bench": "resample", "shape": name, "B": B, "samples_in": L, "samples_out": M, "o": r.o, "n": r.n,
                "W": r.width, "taps": K, "calls": a.calls, "native_ms_median": round(med, 4),
                "native_ms_min": round(best, 4), "native_ms_p90": round(p90, 4), "kernel_ms_mean": round(kern, 4),
                "gflop": round(flop / 1e9, 3),
                "f32_mfma_peak_fraction": round(flop / (med * 1e-3) / F32_MFMA_PEAK, 4),
                "kernel_f32_mfma_peak_fraction": round(flop / (kern * 1e-3) / F32_MFMA_PEAK, 4),
                "mfma_floor_ms": round(flop / F32_MFMA_PEAK * 1e3, 4), "hbm_floor_ms": round(nbytes / HBM_PEAK * 1e3, 4),
                "floor_ms": round(floor_ms, 4), "floor_bound": "mfma" if flop / F32_MFMA_PEAK > nbytes / HBM_PEAK else "hbm",
                "device": torch.cuda.get_device_name(0), "lib": _lib.lib().pd_build_config().decode()}
        if graph_ms is not None:
            line["graph_ms_per_call"] = round(graph_ms, 4)
            line["graph_f32_mfma_peak_fraction"] = round(flop / (graph_ms * 1e-3) / F32_MFMA_PEAK, 4)
        else:
            line["graph_error"] = graph_error
        if not a.no_torch:
            try:
                kernel = r.kernel
                ref = torch_resample(y, kernel, r.width, r.o, r.n, M)
                line["torch_max_abs_diff"] = float((ref - out).abs().max())
                tm, tb, _ = time_calls(lambda: torch_resample(y, kernel, r.width, r.o, r.n, M), a.calls, a.warmup)
                line["torch_ms_median"], line["torch_ms_min"] = round(tm, 4), round(tb, 4)
            except Exception as e:   # conv1d on this build / device
                line["torch_error"] = f"{type(e).__name__}: {e}"[:300]
        print(json.dumps(line), flush=True)
        r.close()


if __name__ == "__main__":
    main()
