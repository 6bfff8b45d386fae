"""Generate the harmonic-noise separation fixtures (tests/golden/vr_*.npz) from the REFERENCE's
modules/vr/nets.py:CascadedNet, run on the CPU in float32 and in float64.

Runs only where the reference checkout exists; PRODIFF_REFERENCE names its root:

    PRODIFF_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_vr.py

Each fixture holds the input ``wav`` [B, C, L], the float32 run's ``spec`` and ``mask`` (complex64
[B, C, n_fft/2 + 1, T]) and ``y`` [B, C, L] of ``predict_from_audio``, the float64 run's ``y64`` and ``mask64``
(the same weights and input cast to double; the whole mask for the three small cases, the fixed positions
``mask64_pos`` of tests/vr_cases.py:subset_positions for the two full-size ones), the ordered state-dict key list and
the seeds.  No weights are stored: they come from prodiff_amd.synth by seed (tests/vr_cases.py).
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ["PRODIFF_REFERENCE"]
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

from tests import golden_io          # noqa: E402
from tests import vr_cases as VC     # noqa: E402

pkg = types.ModuleType("modules.vr")     # modules/vr/__init__.py itself is not needed (and imports yaml)
pkg.__path__ = [os.path.join(REF, "modules", "vr")]
sys.modules["modules.vr"] = pkg
torch.set_num_threads(8)

from modules.vr.nets import CascadedNet   # noqa: E402


def run(net, wav):
    """predict_from_audio with its spectrum and mask kept."""
    seen = {}
    fwd = net.forward

    def keep(spec):
        seen["spec"] = spec
        seen["mask"] = fwd(spec)
        return seen["mask"]

    net.forward = keep
    try:
        with torch.no_grad():
            y = net.predict_from_audio(wav)
    finally:
        del net.forward
    return seen["spec"].numpy(), seen["mask"].numpy(), y.numpy()


def main():
    for name in VC.CASES:
        n_fft, hop, nout, nout_lstm, mono, B, L, pseed, iseed = VC.CASES[name]
        params = VC.case_params(name)
        net = CascadedNet(n_fft, hop, nout, nout_lstm, True, mono).eval()
        keys = list(net.state_dict())
        net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=False)
        wav = VC.case_wav(name)
        spec, mask, y = run(net, torch.from_numpy(wav))
        net64 = net.double()
        _, mask64, y64 = run(net64, torch.from_numpy(wav).double())
        T = VC.frames_of(name)[0]
        assert spec.shape == (B, 1 if mono else 2, n_fft // 2 + 1, T) and T == VC.FRAMES[name], spec.shape
        mag = np.abs(mask64)
        sat = float((mag > 0.999).mean())
        assert sat < 0.01, (name, sat)
        arrays = dict(wav=wav, spec=spec.astype(np.complex64), mask=mask.astype(np.complex64), y=y.astype(np.float32),
                      y64=y64, keys=np.array(keys), param_seed=np.int64(pseed), input_seed=np.int64(iseed))
        if name in VC.SMALL:
            arrays["mask64"] = mask64
        else:
            pos = VC.subset_positions(name, mask64.shape)
            arrays["mask64_pos"] = pos
            arrays["mask64"] = mask64.reshape(-1)[pos]
        paths = golden_io.save(name, arrays)
        e_mask = float(np.abs(mask - mask64).max())
        e_y = float(np.abs(y - y64).max())
        print(f"{name}: T {T}  |mask| mean {mag.mean():.3f} std {mag.std():.3f} sat {sat:.4f}  e_ref mask {e_mask:.2e} "
              f"y {e_y:.2e}  peak y {np.abs(y64).max():.3f}  files {[os.path.getsize(p) for p in paths]}")


if __name__ == "__main__":
    main()
