"""The harmonic-noise separation cases shared by tests/golden/gen_golden_vr.py and the tests: the smallest shapes at
which the kernels can still go wrong.

  vr_tiny_mono     channel counts 1 to 40, every one padded to a 16-channel chunk; two batch rows, two frame tiles
  vr_tiny_stereo   the four-channel input; one 2-frame column at the bottom of the U-Nets
  vr_odd           widths 3, 6, 9, 18, ...: no multiple of 4, every source takes the scalar loads
  vr_full_t32      the shipped CascadedNet(2048, 512, 32, 128): every real width from 2 to 1280
  vr_full_b2t64    the same with two tile rows at the bottom and a batch
"""
import numpy as np

from prodiff_amd import synth
from prodiff_amd.vr import padded_frames

# name -> (n_fft, hop, nout, nout_lstm, is_mono, B, L, parameter seed, input seed)
CASES = {
    "vr_tiny_mono": (128, 32, 8, 16, True, 2, 32 * 40 + 17, 51, 151),
    "vr_tiny_stereo": (128, 32, 8, 16, False, 1, 32 * 20 + 5, 52, 152),
    "vr_odd": (256, 64, 12, 24, True, 1, 64 * 25 + 3, 53, 153),
    "vr_full_t32": (2048, 512, 32, 128, True, 1, 512 * 20 + 100, 54, 154),
    "vr_full_b2t64": (2048, 512, 32, 128, True, 2, 512 * 40 + 17, 54, 155),
}
FRAMES = {"vr_tiny_mono": 64, "vr_tiny_stereo": 32, "vr_odd": 32, "vr_full_t32": 32, "vr_full_b2t64": 64}
SMALL = ("vr_tiny_mono", "vr_tiny_stereo", "vr_odd")     # the fixtures hold their whole masks
N_SUBSET = 40000                                         # recorded float64 mask positions of the full-size cases


def model_args(name):
    n_fft, hop, nout, nout_lstm, mono = CASES[name][:5]
    return dict(n_fft=n_fft, hop_length=hop, nout=nout, nout_lstm=nout_lstm, is_mono=mono)


def case_params(name):
    n_fft, _, nout, nout_lstm, mono = CASES[name][:5]
    return synth.synth_vr_params(synth.vr_param_shapes(n_fft, nout, nout_lstm, mono), CASES[name][7])


def gliding_signal(n, period, f_start, f_end, seed):
    """Eight gliding partials with 1/k amplitudes plus 10 % noise, float32 [n]; ``period`` = samples per cycle
    of a unit frequency (the sample rate when the frequencies are in Hz)."""
    t = np.arange(n, dtype=np.float64) / period
    f = f_start + (f_end - f_start) * t / max(t[-1], 1e-9)
    phase = 2 * np.pi * np.cumsum(f) / period
    x = sum(np.sin(k * phase) / k for k in range(1, 9))
    x = 0.2 * x + 0.02 * np.random.default_rng(seed).standard_normal(n)
    return x.astype(np.float32)


def case_wav(name):
    """[B, C, L]: every row its own glide and noise, scaled with n_fft so that the partials spread over the bins
    of the small transforms as they do at 44.1 kHz in the full one."""
    n_fft, _, _, _, mono, B, L, _, iseed = CASES[name]
    C = 1 if mono else 2
    period = 44100.0 * n_fft / 2048
    rows = [gliding_signal(L, period, 180.0 + 70.0 * r, 260.0 + 90.0 * r, iseed * 10 + r) for r in range(B * C)]
    return np.stack(rows).reshape(B, C, L)


def subset_positions(name, shape):
    """The fixed flat positions of a full-size case's mask at which the float64 run is recorded."""
    n = int(np.prod(shape))
    return np.sort(np.random.default_rng(CASES[name][8]).choice(n, size=min(N_SUBSET, n), replace=False))


def state_dict_keys(name):
    """The reference state-dict key order the fixtures record, restated: every BatchNorm's num_batches_tracked
    after its running_var."""
    n_fft, _, nout, nout_lstm, mono = CASES[name][:5]
    out = []
    for k in synth.vr_param_shapes(n_fft, nout, nout_lstm, mono):
        out.append(k)
        if k.endswith(".running_var"):
            out.append(k[:-len("running_var")] + "num_batches_tracked")
    return out


def frames_of(name):
    return padded_frames(CASES[name][6], CASES[name][1])
