"""Golden vectors for the variance predictors' encoders, made by running the REFERENCE
``modules/variance_predictor/pitch_predictor.py`` and ``dur_predictor.py`` on the CPU.  Runs only in the
survey container, where ``/root/reference`` exists:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_variance.py

Weights come from ``prodiff_amd.synth`` by seed (tests/variance_cases.py), so the files hold the inputs,
the reference's outputs and its ordered state-dict key list only.  The small cases of tests/encoder_cases.py
(other widths, head counts, kernel sizes and depths) are written the same way as encdims_pitch_* / encdims_dur_*.

* pitch: ``cond`` is what PitchPredictor.forward hands to ``self.diffusion`` (pitch_predictor.py:118-120),
  captured by a forward pre-hook on it; it is deterministic (the draws happen inside the sampler).
* duration: ``log`` is the output of ``dur_pred.linear`` re-masked as tts_modules.py:127 does, captured
  by a forward hook; ``dur`` is what DurPredictor.forward(infer=True) returns.
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
sys.modules.setdefault("chardet", types.ModuleType("chardet"))   # utils/__init__.py:6
torch.set_num_threads(8)

from tests import encoder_cases as EC  # noqa: E402
from tests import golden_io as G  # noqa: E402
from tests import variance_cases as VC  # noqa: E402
from modules.variance_predictor.dur_predictor import DurPredictor  # noqa: E402
from modules.variance_predictor.pitch_predictor import PitchPredictor  # noqa: E402


def load_params(m, P):
    sd = m.state_dict()
    own = [k for k in sd if k in P]
    assert own == list(P), "state-dict order differs from the synth table"
    for k, v in P.items():
        assert tuple(sd[k].shape) == v.shape, (k, sd[k].shape, v.shape)
    missing, unexpected = m.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()}, strict=False)
    assert not unexpected
    assert all(k.startswith("diffusion.") or k.endswith("_float_tensor") for k in missing), missing
    return np.array(list(sd))


def tt(x):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in x.items()}


def pitch_cases():
    """(fixture name, hp, params, inputs, seeds): tests/variance_cases.py, then the small cases of
    tests/encoder_cases.py (encdims_pitch_<name>.npz)."""
    for name, c in VC.PITCH_CASES.items():
        yield name, VC.pitch_hp(name), VC.pitch_params(name), VC.pitch_inputs(name), c
    for name in EC.fixture_cases("pitch"):
        yield (f"encdims_pitch_{name}", EC.hp_of("pitch", name), EC.params("pitch", name), EC.inputs("pitch", name),
               dict(param_seed=EC.seed_of("pitch", name), input_seed=EC.seed_of("pitch", name) + 1))


def dur_cases():
    for name, c in VC.DUR_CASES.items():
        yield name, VC.dur_hp(name), VC.dur_params(name), VC.dur_inputs(name), c
    for name in EC.fixture_cases("dur"):
        yield (f"encdims_dur_{name}", EC.hp_of("dur", name), EC.params("dur", name), EC.inputs("dur", name),
               dict(param_seed=EC.seed_of("dur", name), input_seed=EC.seed_of("dur", name) + 1))


def gen_pitch():
    for name, hp, P, x, c in pitch_cases():
        m = PitchPredictor(VC.VOCAB, VC.reference_pitch_hparams(hp)).eval()
        keys = load_params(m, P)
        got = {}
        hk = m.diffusion.register_forward_pre_hook(lambda mod, a: got.setdefault("cond", a[0].detach().clone()))
        t = tt(x)
        with torch.no_grad():
            m(t["txt_tokens"], t["mel2ph"], t["note_midi"], t["note_rest"], t["mel2note"], t["base_pitch"],
              pitch=t.get("pitch"), pitch_retake=t.get("pitch_retake"), pitch_expr=t.get("pitch_expr"),
              spk_id=t.get("spk_id"), infer_step=1, infer=True)
        hk.remove()
        cond = got["cond"].numpy().astype(np.float32)
        assert cond.shape == x["mel2ph"].shape + (hp["hidden_size"],) and np.isfinite(cond).all()
        if name == "pitchcond_small":
            assert x["mel2ph"].shape[1] <= 160 and x["mel2ph"].shape[1] % 8 != 0
        G.save(name, dict(x, cond=cond, state_dict_keys=keys, param_seed=np.int64(c["param_seed"]),
                          input_seed=np.int64(c["input_seed"]), vocab=np.int64(VC.VOCAB)))
        print(name, cond.shape, float(np.abs(cond).max()))


def gen_dur():
    for name, hp, P, x, c in dur_cases():
        m = DurPredictor(VC.VOCAB, VC.reference_dur_hparams(hp)).eval()
        keys = load_params(m, P)
        got = {}
        hk = m.dur_pred.linear.register_forward_hook(lambda mod, a, out: got.setdefault("lin", out.detach().clone()))
        t = tt(x)
        with torch.no_grad():
            dur = m(t["txt_tokens"], t["onset"], t["word_dur"], infer=True).numpy().astype(np.float32)
        hk.remove()
        nonpad = x["txt_tokens"] != 0
        log = (got["lin"].numpy()[..., 0] * nonpad).astype(np.float32)   # tts_modules.py:127
        pos = int((dur[nonpad] > 0).sum())
        assert 2 * pos >= int(nonpad.sum()), f"{name}: only {pos} of {int(nonpad.sum())} durations are > 0"
        assert np.all(dur[~nonpad] == 0)
        G.save(name, dict(x, log=log, dur=dur, state_dict_keys=keys, param_seed=np.int64(c["param_seed"]),
                          input_seed=np.int64(c["input_seed"]), vocab=np.int64(VC.VOCAB)))
        print(name, dur.shape, f"{pos}/{int(nonpad.sum())} > 0", float(np.abs(log).max()), float(dur.max()))


if __name__ == "__main__":
    gen_pitch()
    gen_dur()
