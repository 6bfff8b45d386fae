"""CPU-only checks of the variance predictors (prodiff_amd.variance, pd_pitch_cond / pd_dur): the parameter
containers carry the reference's state-dict keys in its order, the C-ABI counts agree, create rejects
dims the kernels do not take before touching a device, and the float64 restatement of both forwards
(tests/variance_ref.py) reproduces the reference's own outputs in every fixture."""
import numpy as np
import pytest
import torch

from prodiff_amd import _lib, synth
from tests import variance_cases as VC
from tests import variance_ref as VR

ORACLE_TOL = 5e-5   # tests/test_oracle.py's bound for the cond_* fixtures: the fp32 reference's own rounding


def pitch_model(name):
    from prodiff_amd import PitchPredictor
    return PitchPredictor(VC.VOCAB, VC.reference_pitch_hparams(VC.pitch_hp(name)))


def dur_model(name):
    from prodiff_amd import DurPredictor
    return DurPredictor(VC.VOCAB, VC.reference_dur_hparams(VC.dur_hp(name)))


@pytest.mark.parametrize("name", list(VC.PITCH_CASES))
def test_pitch_state_dict_matches_reference(name):
    hp, P, ins, d = VC.pitch_case(name)
    m = pitch_model(name)
    assert list(m.state_dict()) == [str(k) for k in d["state_dict_keys"]]
    own = [k for k in m.state_dict() if not k.startswith("diffusion.") and not k.endswith("_float_tensor")]
    assert own == list(P) == list(synth.pitch_param_shapes(VC.VOCAB, **hp))
    assert all(tuple(m.state_dict()[k].shape) == v.shape for k, v in P.items())
    ps = m.ordered_cond_params()
    assert _lib.lib().pd_pitch_cond_num_params(_lib.C.byref(m.cond_dims())) == len(ps) == len(P)
    sd = m.state_dict(keep_vars=True)
    assert all(p is sd[k] for p, k in zip(ps, P)), "ordered_cond_params is not the state-dict order"


@pytest.mark.parametrize("name", list(VC.DUR_CASES))
def test_dur_state_dict_matches_reference(name):
    hp, P, ins, d = VC.dur_case(name)
    m = dur_model(name)
    assert list(m.state_dict()) == [str(k) for k in d["state_dict_keys"]]
    own = [k for k in m.state_dict() if not k.endswith("_float_tensor")]
    assert own == list(P) == list(synth.dur_param_shapes(VC.VOCAB, **hp))
    assert all(tuple(m.state_dict()[k].shape) == v.shape for k, v in P.items())
    ps = m.ordered_dur_params()
    assert _lib.lib().pd_dur_num_params(_lib.C.byref(m.dur_dims())) == len(ps) == len(P)
    sd = m.state_dict(keep_vars=True)
    assert all(p is sd[k] for p, k in zip(ps, P)), "ordered_dur_params is not the state-dict order"


def test_containers_load_and_refuse_what_the_reference_cannot_run():
    from prodiff_amd import PitchPredictor
    m = pitch_model("pitchcond_small")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in VC.pitch_params("pitchcond_small").items()}, strict=False)
    with pytest.raises(NotImplementedError):
        m(*[None] * 6, infer=False)
    with pytest.raises(NotImplementedError):
        dur_model("dur_small")(None, None, None, infer=False)
    hp = VC.reference_pitch_hparams(VC.pitch_hp("pitchcond_small"))
    with pytest.raises(ValueError):
        PitchPredictor(VC.VOCAB, dict(hp, use_dur_embed=False))


def test_create_rejects_bad_dims():
    """Before any device call: params is NULL, so a create that got past its dims checks would report the
    null pointer instead -- the error text tells the two apart."""
    lib = _lib.lib()
    h = _lib.C.c_void_p()

    def pitch(*dims):
        rc = lib.pd_pitch_cond_create(_lib.C.byref(_lib.pd_pitch_cond_dims(*dims)), None, 0, None, _lib.C.byref(h))
        return rc, lib.pd_last_error().decode()

    def dur(*dims):
        rc = lib.pd_dur_create(_lib.C.byref(_lib.pd_dur_dims(*dims)), None, 0, None, _lib.C.byref(h))
        return rc, lib.pd_last_error().decode()

    rc, msg = pitch(40, 256, 4, 9, 3, 128, 4, 9, 2, 1, 1)      # 256 / 3 heads
    assert rc == 1 and "num_heads" in msg
    rc, msg = pitch(40, 256, 4, 9, 2, 128, 4, 9, 3, 1, 1)      # note encoder: 128 / 3 heads
    assert rc == 1 and "note encoder" in msg
    rc, msg = pitch(40, 256, 4, 9, 2, 128, 4, 8, 2, 1, 1)      # even note FFN kernel
    assert rc == 1 and "odd" in msg
    rc, msg = pitch(40, 256, 4, 9, 2, 128, 4, 9, 4, 1, 1)      # head dim 32
    assert rc == 4 and "head dim" in msg
    rc, msg = pitch(40, 256, 4, 9, 2, 128, 4, 9, 2, 0, 1)      # use_spk_id without speakers
    assert rc == 1 and "num_spk" in msg
    rc, msg = pitch(40, 256, 4, 9, 2, 128, 4, 9, 2, 1, 1)      # good dims: only the parameters are missing
    assert rc == 1 and "null pointer" in msg
    rc, msg = dur(40, 256, 4, 9, 3, 5, 512, 3, 1.0)            # 256 / 3 heads
    assert rc == 1 and "num_heads" in msg
    rc, msg = dur(40, 256, 4, 9, 2, 5, 512, 4, 1.0)            # even kernel size
    assert rc == 1 and "kernel_size" in msg
    rc, msg = dur(40, 256, 4, 9, 2, 5, 500, 3, 1.0)            # n_chans not a multiple of the GEMM's K step (32)
    assert rc == 1 and "n_chans" in msg
    rc, msg = dur(40, 256, 4, 9, 2, 5, 512, 3, 1.0)
    assert rc == 1 and "null pointer" in msg
    assert h.value is None


def test_wavenet_create_rejects_bad_dims():
    """pd_wavenet_create checks its dims before its parameter list, as the creates above: with params NULL every
    bad dim reports its own message, and only good dims get as far as the null pointer.  min(L, cycle) = 32
    would dilate a layer by 2^31."""
    lib = _lib.lib()
    h = _lib.C.c_void_p()

    def wavenet(*dims):
        rc = lib.pd_wavenet_create(_lib.C.byref(_lib.pd_wavenet_dims(*dims)), None, 0, None, _lib.C.byref(h))
        return rc, lib.pd_last_error().decode()

    for dims, word in (((6, 256, 20, 256, 1), "in_dims"), ((80, 10, 20, 256, 1), "hidden_size"),
                       ((80, 256, 20, 48, 1), "residual_channels"), ((80, 256, 0, 256, 1), "residual_layers"),
                       ((80, 256, 20, 256, 0), "dilation_cycle_length must be positive"),
                       ((80, 256, 32, 256, 32), "dilation_cycle_length: a dilation")):
        rc, msg = wavenet(*dims)
        assert rc == 1 and word in msg and "null pointer" not in msg, (dims, rc, msg)
    for dims in ((80, 256, 20, 256, 1), (12, 36, 3, 96, 3), (80, 256, 31, 256, 40), (80, 256, 40, 256, 31)):
        rc, msg = wavenet(*dims)
        assert rc == 1 and "null pointer" in msg, (dims, rc, msg)
    assert h.value is None


@pytest.mark.parametrize("name", list(VC.PITCH_CASES))
def test_pitch_ref_matches_reference(name):
    hp, P, ins, d = VC.pitch_case(name)
    cond = VR.pitch_condition(P, hp, **ins)
    err = float(np.abs(cond - d["cond"]).max())
    print(f"PITCHREF {name} max|d|={err:.3e} max|cond|={np.abs(d['cond']).max():.3f}", flush=True)
    assert err <= ORACLE_TOL
    # the reference has no final mel2ph > 0 mask: padding frames keep the speaker / retake / delta terms
    pad = d["mel2ph"] == 0
    if pad.any():
        assert np.abs(d["cond"][pad]).max() > 0


@pytest.mark.parametrize("name", list(VC.DUR_CASES))
def test_dur_ref_matches_reference(name):
    hp, P, ins, d = VC.dur_case(name)
    dur, log = VR.dur_forward(P, hp, **ins)
    e_log = float(np.abs(log - d["log"]).max())
    e_dur = float((np.abs(dur - d["dur"]) / np.maximum(1.0, np.abs(d["dur"]))).max())
    print(f"DURREF {name} log max|d|={e_log:.3e} dur rel={e_dur:.3e}", flush=True)
    assert e_log <= ORACLE_TOL and e_dur <= ORACLE_TOL
    nonpad = d["txt_tokens"] != 0
    assert np.all(d["dur"][~nonpad] == 0) and np.all(d["log"][~nonpad] == 0)
    assert 2 * int((d["dur"][nonpad] > 0).sum()) >= int(nonpad.sum())   # the clamp does not hide the head


def test_fixture_inputs_come_from_synth():
    """The stored inputs are what synth draws from the stored seeds (the generator and the tests agree)."""
    for name in VC.PITCH_CASES:
        d = VC.pitch_case(name)[3]
        for k, v in VC.pitch_inputs(name).items():
            assert np.array_equal(d[k], v), (name, k)
    for name in VC.DUR_CASES:
        d = VC.dur_case(name)[3]
        for k, v in VC.dur_inputs(name).items():
            assert np.array_equal(d[k], v), (name, k)
