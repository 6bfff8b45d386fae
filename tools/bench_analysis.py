#!/usr/bin/env python
"""Time FastDiff's native analysis (prodiff_amd.analysis: the BS.1770 meter's six launches, the padding, the
zero-padded centred mel) with HIP events: warm-up, then the median over --calls single calls, for one clip of
--seconds at 22.05 kHz and for a ragged batch of 8 (device tensors in and out, so no transfer is timed).  Beside it
the host chain the reference runs, restated with scipy and numpy in float64 (tests/analysis_ref.py: lfilter, the
block loop, np.fft), timed with the wall clock over --host-calls calls.  Prints one JSON line per shape.

    python tools/bench_analysis.py [--calls 100] [--warmup 10] [--seconds 10]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from prodiff_amd import _lib  # noqa: E402
from prodiff_amd import analysis as A  # noqa: E402
from tests import analysis_ref as R  # noqa: E402

RATE = 22050


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
    return round(float(np.median(ms)), 4), round(float(ms[0]), 4), round(float(ms[int(0.9 * (len(ms) - 1))]), 4)


def host_ms(fn, calls):
    fn()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(t)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--host-calls", type=int, default=3)
    a = ap.parse_args()
    assert a.calls >= 50, "median over at least 50 calls"
    dev = torch.device("cuda:0")
    L = int(a.seconds * RATE)
    for B in (1, 8):
        lens = [L - 1237 * i for i in range(B)]
        clips = [R.make_signal("harmonic", n, RATE, 50 + i) for i, n in enumerate(lens)]
        batch = torch.zeros(B, L)
        for i, c in enumerate(clips):
            batch[i, :lens[i]] = torch.from_numpy(c)
        batch = batch.to(dev)
        kw = dict(vocoder="fastdiff", eps=1e-10, to_numpy=False, lens=lens, **R.TTS)
        loud = A.integrated_loudness(batch, RATE, lens=lens)
        line = {"bench": "analysis", "B": B, "samples": L, "rate": RATE, "frames": 1 + L // R.TTS["hop_size"],
                "calls": a.calls, "chunk": _lib.lib().pd_loudness_chunk(),
                "loudness_max_abs_diff_db": float(max(abs(float(loud[i]) - R.integrated_loudness64(c, RATE))
                                                      for i, c in enumerate(clips))),
                "device": torch.cuda.get_device_name(0), "lib": _lib.lib().pd_build_config().decode()}
        for key, fn in (("loudness", lambda: A.integrated_loudness(batch, RATE, lens=lens)),
                        ("process_utterance_loud_norm", lambda: A.process_utterance(batch, loud_norm=True, **kw)),
                        ("process_utterance_plain", lambda: A.process_utterance(batch, loud_norm=False, **kw))):
            med, best, p90 = time_calls(fn, a.calls, a.warmup)
            line[f"{key}_ms_median"], line[f"{key}_ms_min"], line[f"{key}_ms_p90"] = med, best, p90
        line["host_loudness_ms"] = host_ms(lambda: [R.integrated_loudness64(c, RATE) for c in clips], a.host_calls)
        line["host_process_utterance_loud_norm_ms"] = host_ms(
            lambda: [R.process_utterance64(c, loud_norm=True, vocoder="fastdiff", eps=1e-10, **R.TTS) for c in clips],
            a.host_calls)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
