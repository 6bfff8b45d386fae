"""Timing of the variance predictors' encoders on the GPU: PitchPredictor.forward_condition
(pd_pitch_cond_forward) and DurPredictor (pd_dur_forward) at the shipped configuration.

    python tools/bench_variance.py [--frames 861] [--tokens 120] [--notes 60] [--dtype fp32|bf16] [--iters 50]

Synthetic handler-config models (H=256, 4 FFT layers, 2 heads, k=9; note encoder 128 x 4; duration
predictor 5 x 512, k=3), N phonemes and notes per utterance over `frames` mel frames, for B = 1 and
B = 8.  Prints one JSON line per (stage, batch): HIP-event ms per call (median over --iters, after a
warm-up), and the per-tag launch table of one profiled call."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from prodiff_amd import DurPredictor, PitchPredictor, _lib, synth  # noqa: E402

V = 64
PITCH_HP = dict(hidden_size=256, enc_layers=4, enc_ffn_kernel_size=9, num_heads=2, dropout=0.1, use_dur_embed=True,
                use_spk_id=True, datasets=["a", "b"], sampling_algorithm="euler",
                f0_prediction_args=dict(spec_min=-8.0, spec_max=8.0, clamp_min=-12.0, clamp_max=12.0, repeat_bins=64,
                                        encoder_args=dict(hidden_size=128, num_layers=4, ffn_kernel_size=9,
                                                          num_heads=2),
                                        denoise_args=dict(dilation_cycle_length=5, residual_layers=1,
                                                          residual_channels=64),
                                        timesteps=4, timescale=1000))
DUR_HP = dict(hidden_size=256, enc_layers=4, enc_ffn_kernel_size=9, num_heads=2,
              dur_prediction_args=dict(num_layers=5, hidden_size=512, dropout=0.1, kernel_size=3, log_offset=1.0,
                                       loss_type="mse"))


def event_ms(fn, iters):
    """Median HIP-event time of fn() over `iters` calls, each bracketed by its own event pair."""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):   # back to back: what a caller that does not wait between calls sees
        fn()
    b.record()
    b.synchronize()
    return statistics.median(ts), min(ts), a.elapsed_time(b) / iters


def launches(fn):
    _lib.profile_enable(True)
    fn()
    torch.cuda.synchronize()
    prof = _lib.profile_summary()
    _lib.profile_enable(False)
    return ({k: round(v[1] * 1e3 / v[0], 2) for k, v in prof.items()}, {k: v[0] for k, v in prof.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=861)
    ap.add_argument("--tokens", type=int, default=120)
    ap.add_argument("--notes", type=int, default=60)
    ap.add_argument("--dtype", default="fp32")
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    cuda = lambda x: {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in x.items()}
    pm = PitchPredictor(V, PITCH_HP)
    pp = synth.synth_variance_params(synth.pitch_param_shapes(V, num_spk=2), 0)
    pm.load_state_dict({k: torch.from_numpy(v) for k, v in pp.items()}, strict=False)
    pm = pm.cuda().set_compute_dtype(a.dtype)
    dm = DurPredictor(V, DUR_HP)
    dp = synth.synth_variance_params(synth.dur_param_shapes(V), 1)
    dm.load_state_dict({k: torch.from_numpy(v) for k, v in dp.items()}, strict=False)
    dm = dm.cuda().set_compute_dtype(a.dtype)
    for B in (1, 8):
        px = cuda(synth.synth_pitch_inputs(7, [a.tokens] * B, [a.notes] * B, V, 2, frames=a.frames))
        dx = cuda(synth.synth_dur_inputs(8, [a.tokens] * B, V))
        for what, fn in (("PitchPredictor.forward_condition", lambda: pm.forward_condition(**px)),
                         ("DurPredictor.forward", lambda: dm(**dx))):
            med, best, window = event_ms(fn, a.iters)
            us, n = launches(fn)
            print(json.dumps({"what": what, "dtype": a.dtype, "batch": B, "tokens": a.tokens, "notes": a.notes,
                              "mel_frames": a.frames, "ms_per_call": round(med, 4), "ms_best": round(best, 4), "ms_back_to_back": round(window, 4),
                              "launches_total": sum(n.values()), "kernels_us": us, "launches": n}), flush=True)


if __name__ == "__main__":
    main()
