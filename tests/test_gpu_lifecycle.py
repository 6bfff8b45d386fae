"""Lifecycle of the four native handles (WaveNet, FastDiff, NSF-HiFiGAN, condition encoder) on the
GPU, at the smallest shapes that reach every device allocation a create makes: the weight pool,
its bf16 mirror, WaveNet's fragment-order buffer (M=80, H=256, C=256 in bf16 only) and FastDiff's
pre-scaled kernel-predictor weights (bf16).

``pd_live_device_bytes`` counts what the live handles of this process hold, so every check is a
difference against the count at the test's start (other tests' modules may still be alive).
"""
import gc

import numpy as np
import pytest
import torch

from prodiff_amd import FastDiff, WaveNet, _lib, synth
from tests import golden_io as G
from tests.nsf_cases import load as nsf_load
from tests.test_gpu_cond import cuda_inputs, teacher_for

pytestmark = pytest.mark.gpu
DEV = "cuda"


def tt(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def live():
    return _lib.lib().pd_live_device_bytes()


class Case:
    """make() -> a fresh module on the GPU; run(m) -> one forward's output; pack(m) -> its handle;
    option: a valid non-default kernel option (None: the component has none)."""
    option = None

    def pack(self, m):
        return m.handle()


class WaveNetCase(Case):
    dtype, option = "bf16", {"layer": 0}

    def make(self):
        m = WaveNet(80, 256, 2, 256, 1)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in
                           synth.synth_params(synth.wavenet_param_shapes(80, 256, 2, 256), 3).items()})
        return m.to(DEV)

    def run(self, m):
        return m(tt(synth.synth_inputs(1, (1, 1, 80, 64))), tt(np.array([2.0], np.float32)),
                 tt(synth.synth_inputs(2, (1, 256, 64))))


class FastDiffCase(Case):
    dtype, option = "bf16", {"lvc_pf": 0}

    def make(self):
        m = FastDiff()
        m.load_state_dict({k: torch.from_numpy(v) for k, v in
                           synth.synth_params(synth.fastdiff_param_shapes(), 31).items()})
        return m.to(DEV)

    def run(self, m):
        Tc = 16
        return m((tt(synth.synth_inputs(3, (1, 1, Tc * 256))), tt(synth.synth_inputs(4, (1, 80, Tc), loc=-5.0, scale=2.0)),
                  tt(np.array([[23.4676]], np.float32))))


class NsfCase(Case):
    dtype, option = "bf16", {"wconv": 0}

    def make(self):
        from prodiff_amd.nsf_hifigan import Generator
        h, self.io, seed = nsf_load("nsf_c32_r44_rb2")
        m = Generator(h)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in
                           synth.synth_params(synth.nsf_param_shapes(**h), seed).items()})
        return m.to(DEV).eval()

    def run(self, m):
        io = self.io
        return m.synthesize(tt(io["mel"]), tt(io["f0"]), 2.30259, rand_ini=tt(io["rand_ini"]), noise=tt(io["noise"]))


class CondCase(Case):
    def __init__(self, dtype):
        self.dtype = dtype

    def make(self):
        hp, P, self.ins, d = G.cond_case("cond_small")
        return teacher_for(hp, P, int(d["vocab"]))

    def pack(self, m):
        return m.cond_handle()

    def run(self, m):
        x = cuda_inputs(self.ins)
        return m.forward_condition(x.pop("txt_tokens"), x.pop("mel2ph"), x.pop("f0"), **x)


CASES = {"wavenet": WaveNetCase(), "fastdiff": FastDiffCase(), "nsf": NsfCase(), "cond_bf16": CondCase("bf16"),
         "cond_fp32": CondCase("fp32")}


@pytest.fixture(autouse=True)
def _collect_first():
    gc.collect()   # modules that earlier tests dropped give their handles back now, not mid-test


@pytest.mark.parametrize("name", list(CASES))
def test_create_run_close_returns_every_byte(name):
    case = CASES[name]
    base = live()
    for _ in range(5):
        m = case.make().set_compute_dtype(case.dtype)
        h = case.pack(m)
        held = live() - base
        assert held > 0
        assert case.pack(m) is h and live() - base == held     # same signature: the same handle
        out = case.run(m)
        assert case.pack(m) is h and live() - base == held and torch.isfinite(out).all()
        m._native.close()
        assert live() == base
        assert m._native.h is None
    del m
    gc.collect()
    assert live() == base


def _set_dtype(case, m):
    m.set_compute_dtype("fp32" if case.dtype == "bf16" else "bf16")


def _set_option(case, m):
    m.set_options(**case.option)


def _add_to_parameter(case, m):
    with torch.no_grad():
        next(m.parameters()).add_(0.01)


# the condition encoder has no kernel options
CHANGES = [(n, ch) for n, c in CASES.items() for ch in (_set_dtype, _set_option, _add_to_parameter)
           if ch is not _set_option or c.option is not None]


@pytest.mark.parametrize("name,change", CHANGES, ids=[f"{n}-{ch.__name__.strip('_')}" for n, ch in CHANGES])
def test_change_packs_one_new_handle(name, change):
    case = CASES[name]
    base = live()
    m = case.make().set_compute_dtype(case.dtype)
    first = case.run(m)
    h = case.pack(m)
    old = h.value
    change(case, m)
    h2 = case.pack(m)
    assert h2 is not h and h2.value != old        # built before the old one was closed
    held = live() - base
    # a freshly built module in the same state: as many bytes, the same output bit for bit
    f = case.make().set_compute_dtype(case.dtype)
    f.load_state_dict(m.state_dict())
    if change is not _add_to_parameter:           # (that one came with the state dict)
        change(case, f)
    case.pack(f)
    assert live() - base == 2 * held              # one handle each, not the old one as well
    out = case.run(m)
    assert torch.equal(out, case.run(f))
    if change is not _set_option:                 # (another kernel variant may give the same result)
        assert not torch.equal(out, first)
    m._native.close()
    f._native.close()
    assert live() == base
