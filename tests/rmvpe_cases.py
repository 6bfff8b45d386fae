"""The RMVPE parity cases shared by tests/golden/gen_golden_rmvpe.py and the tests: the smallest shapes at which
the kernels can still go wrong.

  rmvpe_shallow   T not a multiple of 32, five pooled rows (odd), one block per level: every block has a 1x1 shortcut
  rmvpe_nogru     the Linear-only head
  rmvpe_slim      one pixel row at the bottom, the transposed conv from a 1 x 4 map, identity-shortcut blocks
  rmvpe_full_*    the shipped E2E0(4, 1, (2, 2)): 2 and 3 bottom rows, every channel width from 16 to 512
"""
import numpy as np

from prodiff_amd import synth

N_MELS, N_CLASS = synth.RMVPE_N_MELS, synth.RMVPE_N_CLASS
CONST = 1997.3794084376191      # modules/rmvpe/constants.py

FULL = dict(n_blocks=4, n_gru=1, en_de_layers=5, inter_layers=4, en_out_channels=16)

# name -> (model arguments, B, T, parameter seed, input seed)
CASES = {
    "rmvpe_shallow": (dict(n_blocks=1, n_gru=1, en_de_layers=2, inter_layers=1, en_out_channels=16), 2, 20, 41, 141),
    "rmvpe_nogru": (dict(n_blocks=1, n_gru=0, en_de_layers=3, inter_layers=1, en_out_channels=16), 1, 40, 42, 142),
    "rmvpe_slim": (dict(n_blocks=2, n_gru=1, en_de_layers=5, inter_layers=2, en_out_channels=16), 2, 32, 43, 143),
    "rmvpe_full_b2t64": (FULL, 2, 64, 44, 144),
    "rmvpe_full_b1t96": (FULL, 1, 96, 44, 145),
}


def case_mel(name):
    """The case's input: a log-mel-like image [B, N_MELS, T] (natural-log magnitudes around -4)."""
    _, B, T, _, iseed = CASES[name]
    return synth.synth_inputs(iseed, (B, N_MELS, T), loc=-4.0, scale=2.0)


def case_params(name):
    model, _, _, pseed, _ = CASES[name]
    return synth.synth_rmvpe_params(synth.rmvpe_param_shapes(**model), pseed)


def state_dict_keys(model):
    """The reference state-dict key order the fixtures record, restated: the used keys with every BatchNorm's
    num_batches_tracked after its running_var, and unet.tf.* between the intermediate and the decoder."""
    used = list(synth.rmvpe_param_shapes(**model))
    out = []
    for k in used:
        if k.startswith("unet.decoder.layers.0.conv1.0.") and not any(o.startswith("unet.tf.") for o in out):
            for i in range(model["en_de_layers"]):
                p = f"unet.tf.layers.{i}"
                for q in ("conv.0.weight", "conv.1.weight", "conv.1.bias", "conv.1.running_mean", "conv.1.running_var",
                          "conv.1.num_batches_tracked", "conv.3.weight", "conv.4.weight", "conv.4.bias",
                          "conv.4.running_mean", "conv.4.running_var", "conv.4.num_batches_tracked"):
                    out.append(f"{p}.{q}")
        out.append(k)
        if k.endswith(".running_var"):
            out.append(k[:-len("running_var")] + "num_batches_tracked")
    return out


def used_keys(keys):
    return [k for k in keys if not synth.rmvpe_key_is_skipped(k)]


def harmonic_signal(sr, seconds, f_start=180.0, f_end=260.0, seed=7):
    """A gliding harmonic tone with a little noise, float32 [n]: eight partials with 1/k amplitudes."""
    n = int(round(sr * seconds))
    t = np.arange(n, dtype=np.float64) / sr
    f = f_start + (f_end - f_start) * t / max(t[-1], 1e-9)
    phase = 2 * np.pi * np.cumsum(f) / sr
    x = sum(np.sin(k * phase) / k for k in range(1, 9))
    x = 0.2 * x + 0.002 * np.random.default_rng(seed).standard_normal(n)
    return x.astype(np.float32)
