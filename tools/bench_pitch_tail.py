#!/usr/bin/env python
"""Time the pitch extractor's tail with HIP events: pd_rmvpe_viterbi (log-probability pre-pass, forward pass with
its in-kernel backtrace) and pd_f0_align, for 1 x 10 s and 8 x 10 s of salience (T = 1001 frames of 360 classes),
beside pd_rmvpe_decode and beside the host path they replace (device -> host copy, the numpy restatement of
librosa's Viterbi / of interp_f0 + resample_align_curve, host -> device copy).  Warm-up, then the median over
--calls single calls; a per-kernel table from pd_profile_*; the chain replayed from one captured graph.  Prints
one JSON line per shape.

    python tools/bench_pitch_tail.py [--calls 100] [--warmup 5] [--seconds 10] [--batches 1,8] [--no-host]
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
from prodiff_amd import rmvpe as RM  # noqa: E402
from tests import viterbi_ref as V  # noqa: E402

HOP, RATE = 512, 44100          # the mel grid the f0 is aligned to


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


def salience(B, T, seed):
    """A gliding ridge on a noise floor, with random frames every eighth frame (the recurrence's cost does not
    depend on the values; the host path's does not either)."""
    h = np.stack([V.case("glide", T, seed=seed + b) for b in range(B)])
    rng = np.random.default_rng(seed)
    h[:, ::8] = rng.random(h[:, ::8].shape, dtype=np.float32)
    return h


def host_viterbi(hidden_dev):
    """What a caller without the kernel does: the salience to the host, the dense recurrence in numpy, the path back."""
    h = hidden_dev.cpu().numpy()
    paths = np.stack([V.dense(h[b])[1] for b in range(h.shape[0])])
    return torch.from_numpy(paths).to(hidden_dev.device)


def host_tail(f0_dev, length):
    f0 = f0_dev.cpu().numpy()
    outs = [V.align_f0(f0[b], 0.01, HOP / RATE, length) for b in range(f0.shape[0])]
    f = torch.from_numpy(np.stack([o[0] for o in outs])).to(f0_dev.device)
    uv = torch.from_numpy(np.stack([o[1] for o in outs])).to(f0_dev.device)
    return f, uv


def wall_ms(fn, reps):
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    T = int(round(a.seconds * 100)) + 1
    length = int(a.seconds * RATE / HOP)
    for B in [int(x) for x in a.batches.split(",")]:
        hidden = torch.from_numpy(salience(B, T, a.seed)).to(dev)
        line = {"bench": "pitch_tail", "B": B, "T": T, "n_class": hidden.shape[2], "length": length, "calls": a.calls,
                "chunk": RM.VITERBI_CHUNK, "device": torch.cuda.get_device_name(0),
                "lib": _lib.lib().pd_build_config().decode()}
        path = RM.viterbi_path(hidden)
        f0 = RM.to_local_average_f0(hidden, center=path)
        f0[:, T // 3:T // 2] = 0                       # an unvoiced stretch for the tail to fill
        for key, fn in (("viterbi", lambda: RM.viterbi_path(hidden)),
                        ("decode", lambda: RM.to_local_average_f0(hidden)),
                        ("decode_with_path", lambda: RM.to_local_average_f0(hidden, center=path)),
                        ("align", lambda: RM.align_f0(f0, 0.01, HOP / RATE, length))):
            med, best, p90 = time_calls(fn, a.calls, a.warmup)
            line[key + "_ms_median"], line[key + "_ms_min"], line[key + "_ms_p90"] = round(med, 4), round(best, 4), round(p90, 4)

        def chain():
            p = RM.viterbi_path(hidden)
            return RM.align_f0(RM.to_local_average_f0(hidden, center=p), 0.01, HOP / RATE, length)

        eager = chain()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = chain()
        gm, gb, _ = time_calls(graph.replay, a.calls, a.warmup)
        line.update(chain_ms_median=round(time_calls(chain, a.calls, a.warmup)[0], 4), graph_ms_median=round(gm, 4),
                    graph_ms_min=round(gb, 4), graph_equals_eager=bool(torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])))
        n_prof = 10
        _lib.profile_enable(True)
        for _ in range(n_prof):
            chain()
        torch.cuda.synchronize()
        prof = _lib.profile_summary()
        _lib.profile_enable(False)
        line["kernels_ms_per_call"] = {k: [c // n_prof, round(t / n_prof, 4)] for k, (c, t) in sorted(prof.items())}
        if "viterbi_forward" in prof:
            line["forward_us_per_frame"] = round(prof["viterbi_forward"][1] / n_prof / T * 1e3, 4)
        # row 0's shader-cycle stamps at the end of the workspace: the whole forward kernel, its backtrace parts
        RM.viterbi_path(hidden)
        total = _lib.lib().pd_rmvpe_viterbi_workspace_size(B, T, hidden.shape[2], 30)
        buf = RM._VITERBI_WS.bufs[(str(hidden.device), torch.cuda.current_stream(dev).cuda_stream)]
        cyc = buf[total - 16:total].view(torch.int64).cpu().tolist()
        line.update(forward_cycles=cyc[0], backtrace_cycles=cyc[1], backtrace_share=round(cyc[1] / cyc[0], 4))
        if not a.no_host:
            line["host_path_equals_native"] = bool(torch.equal(host_viterbi(hidden), path))
            hv = wall_ms(lambda: host_viterbi(hidden), 2)
            ht = wall_ms(lambda: host_tail(f0, length), 5)
            line.update(host_viterbi_ms=round(hv, 2), host_tail_ms=round(ht, 3),
                        host_over_native_viterbi=round(hv / line["viterbi_ms_median"], 1),
                        host_over_native_tail=round(ht / line["align_ms_median"], 1))
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
