"""Generate the RMVPE fixtures (tests/golden/rmvpe_*.npz) from the REFERENCE's modules/rmvpe/model.py:E2E0,
run on the CPU in float32 and in float64.

Runs only where the reference checkout exists (REF below):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_rmvpe.py

modules/rmvpe/__init__.py imports librosa (not installed there) through spec.py and utils.py, so a stub
package stands in for it and model.py, deepunet.py, seq.py and constants.py are imported as its submodules.

Each fixture holds the input mel [B, 128, T], ``feat`` [B, T, 384] (a forward hook on ``cnn``, transposed and
flattened as model.py:30 does) and ``hidden`` [B, T, 360] of the float32 run, their float64 counterparts
(``feat64``, ``hidden64``: the same weights cast to double), the ordered state-dict key list and the seeds.
No weights are stored: they come from prodiff_amd.synth by seed (tests/rmvpe_cases.py).
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

from tests import golden_io            # noqa: E402
from tests import rmvpe_cases as RC    # noqa: E402

pkg = types.ModuleType("modules.rmvpe")
pkg.__path__ = [os.path.join(REF, "modules", "rmvpe")]
sys.modules["modules.rmvpe"] = pkg
torch.set_num_threads(8)

from modules.rmvpe.model import E2E0   # noqa: E402


def build(model, params, dtype):
    net = E2E0(model["n_blocks"], model["n_gru"], (2, 2), model["en_de_layers"], model["inter_layers"], 1,
               model["en_out_channels"]).eval()
    keys = list(net.state_dict())
    missing = [k for k in RC.used_keys(keys) if k not in params]
    extra = [k for k in params if k not in keys]
    assert not missing and not extra, (missing[:4], extra[:4])
    res = net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=False)
    assert all(RC.synth.rmvpe_key_is_skipped(k) for k in res.missing_keys), res.missing_keys[:4]
    return net.to(dtype), keys


def run(net, mel):
    seen = []
    hook = net.cnn.register_forward_hook(lambda m, i, o: seen.append(o.transpose(1, 2).flatten(-2)))
    try:
        with torch.no_grad():
            hidden = net(mel)
    finally:
        hook.remove()
    return seen[0].numpy(), hidden.numpy()


def run_case(name):
    model, B, T, pseed, iseed = RC.CASES[name]
    params = RC.case_params(name)
    mel = RC.case_mel(name)
    net32, keys = build(model, params, torch.float32)
    assert keys == RC.state_dict_keys(model), "tests/rmvpe_cases.state_dict_keys differs from the reference"
    assert list(params) == RC.used_keys(keys)
    feat, hidden = run(net32, torch.from_numpy(mel))
    net64, _ = build(model, params, torch.float64)
    feat64, hidden64 = run(net64, torch.from_numpy(mel).double())
    assert hidden.shape == (B, T, RC.N_CLASS) and feat.shape == (B, T, 3 * RC.N_MELS)
    out = dict(mel=mel, feat=feat, hidden=hidden, feat64=feat64, hidden64=hidden64, keys=np.array(keys),
               param_seed=np.int64(pseed), input_seed=np.int64(iseed))
    paths = golden_io.save(name, out)
    for p in paths:
        assert os.path.getsize(p) < (1 << 20), (p, os.path.getsize(p))
    top = np.sort(hidden64, axis=-1)
    print(f"{name}: feat peak {np.abs(feat).max():.3g}  e_ref hidden {np.abs(hidden - hidden64).max():.2e} "
          f"feat {np.abs(feat - feat64).max():.2e}  salience range [{hidden.min():.3g}, {hidden.max():.3g}]  "
          f"frames with top-two margin < 2e-4: {np.mean(top[..., -1] - top[..., -2] < 2e-4):.1%}  {len(paths)} file(s)")


def check_f0_condition():
    """The end-to-end f0 test leaves out the frames whose top-two salience margin is below 2e-4 and may leave out
    at most 10 %: with the chosen seed and final-Linear gain (synth.RMVPE_FC_GAIN) the reference's own float32
    run on the test's signals must stay under 5 %."""
    from prodiff_amd.mel import mel_filterbank
    from tests import resample_ref as RR
    from tests import rmvpe_ref as R
    net, _ = build(RC.FULL, RC.case_params("rmvpe_full_b2t64"), torch.float32)
    basis = mel_filterbank(16000, 1024, 128, 30, 8000, htk=True)
    for sr in (16000, 44100):
        x = RC.harmonic_signal(sr, 0.5).astype(np.float64)[None]
        if sr != 16000:
            h, W, o, n = RR.table64(sr, 16000, lowpass_filter_width=128)
            x = RR.direct64(x, h, W, o, n)
        logmel = R.centered_mel(x, basis)[2].astype(np.float32)
        T = logmel.shape[1]
        mel = np.pad(logmel, ((0, 0), (0, -T % 32), (0, 0))).transpose(0, 2, 1)
        with torch.no_grad():
            hidden = net(torch.from_numpy(np.ascontiguousarray(mel))).numpy()[0, :T]
        top = np.sort(hidden, axis=-1)
        close = float(np.mean(top[:, -1] - top[:, -2] < 2e-4))
        print(f"f0 condition at {sr} Hz: {close:.1%} of {T} frames have a top-two margin below 2e-4, "
              f"row maximum in [{top[:, -1].min():.3g}, {top[:, -1].max():.3g}]")
        assert close < 0.05, (sr, close)


if __name__ == "__main__":
    for name in (sys.argv[1:] or RC.CASES):
        run_case(name)
    if not sys.argv[1:]:
        check_f0_condition()
