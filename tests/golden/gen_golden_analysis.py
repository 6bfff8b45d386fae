"""Generate the FastDiff-analysis fixtures (tests/golden/analysis_*.npz): the seeded signals of
tests/analysis_ref.py and what its float64 restatement of pyloudnorm's meter gives for them.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_analysis.py

Neither pyloudnorm nor librosa is installed where this runs, so nothing here comes from the reference's own
run: the restatement is anchored outside itself by tests/test_analysis_cpu.py (the BS.1770-4 coefficient tables
at 48 kHz, the recommendation's 997 Hz conformance reading).

Each fixture holds the wav [L], the rate, the recorded loudness, the block energies z_j, the relative threshold
and the two gates' masks.  Before anything is written, every fixture is checked to keep all its blocks at least
analysis_ref.GATE_MARGIN dB away from both gates: nearer than that, a rounding difference flips a block in or out
and a flip, not an error, decides the result.  The gate fixture must lose blocks to each gate, the clicks fixture
must take the peak branch and the others must not.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import analysis_ref as R  # noqa: E402


def main():
    for name, (rate, L, kind) in R.LOUD_CASES.items():
        wav = R.case_wav(name)
        assert wav.shape == (L,) and wav.dtype == np.float32 and np.abs(wav).max() <= 1.0
        d = R.loudness_detail(wav, rate)
        margin = R.gate_margin(d)
        assert margin >= R.GATE_MARGIN, (name, margin)
        assert np.isfinite(d["loud"]), name
        _, took = R.normalize32(wav, d["loud"], -22.0)
        assert took == (kind == "clicks"), (name, took)
        if kind == "gate":
            silent = ~d["abs_gate"]
            assert silent.any() and (d["abs_gate"] & ~d["rel_gate"]).any() and d["rel_gate"].any(), name
        np.savez(os.path.join(HERE, f"analysis_{name}.npz"), wav=wav, rate=np.int64(rate), loud=np.float64(d["loud"]),
                 z=d["z"], gamma_r=np.float64(d["gamma_r"]), abs_gate=d["abs_gate"], rel_gate=d["rel_gate"],
                 peak_branch=np.bool_(took))
        print(f"{name}: L {L} rate {rate} blocks {len(d['z'])} loud {d['loud']:.6f} gate margin {margin:.3f} dB "
              f"abs {int(d['abs_gate'].sum())} rel {int(d['rel_gate'].sum())} peak branch {took}")


if __name__ == "__main__":
    main()
