"""Which kernels each option selects: the {launch tag: launches} table of one small run per option set of the
three generators, against tests/golden/dispatch_tags.json.

The host code that turns options and shapes into launches can pick another path without changing one output
value (the variants are bit-identical by design, tests/test_gpu_bf16.py, tests/test_gpu_nsf.py); this table is
what notices.  The fixture is recorded with the library of the commit BEFORE a change to that host code:

    tools/build_rev_lib.sh <rev>
    PRODIFF_HIP_LIB=tools/bin/lib_<rev>.so python -m tests.test_gpu_dispatch [out.json]

What the table cannot see: options that choose between kernels launched under one tag leave their row equal to
the default's.  Those are FD_OPT_LVC_PS, LVC_TPW, LVC_PF, LVC_PRIO and the tile sizes LVC_TS 128 / 256
(all fd_lvc_block_*), NSF_OPT_RB16 1 against 2, NSF_OPT_C256 and NSF_OPT_NC_MFMA (nsf_rb16, nsf_res,
nsf_noise_conv), PD_WN_OPT_STACK_RO and stack sizes of 10 and more (wn_stack), and the fp32 WaveNet layers as
kernels or GEMMs (wn_gate / wn_resskip; only the sampler's wn_f32_tail tells them apart).  For those the
bit-exactness tests of the variants remain the only check.

Shapes: two utterances of unequal length, a little over one tile (T >= 64 takes the WaveNet stack kernel, T = 37
does not; 3 mel frames are two 384-row tiles of the last LVC block); every run takes milliseconds.
"""
import json
import os

import numpy as np
import pytest
import torch

from prodiff_amd import FastDiff, GaussianDiffusion, WaveNet, _lib, synth
from prodiff_amd.nsf_hifigan import Generator
from prodiff_amd.schedules import fastdiff_infer_params, fastdiff_reverse_schedule, fastdiff_train_alpha
from tests import golden_io as G

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dispatch_tags.json")

# every non-default value tests/test_gpu_bf16.py and tests/test_gpu_nsf.py set (and PD_WN_OPT_F32_LAYER of
# tests/test_gpu_parity.py), after the defaults
FD_OPTS = [{}, dict(lvc_ts=0), dict(lvc_ts=128), dict(lvc_ts=256),
           dict(lvc_fuse=0, lvc_sub=0, lvc_ts=128), dict(lvc_fuse=0, lvc_sub=0, lvc_ts=256),
           dict(lvc_fuse=0, lvc_sub=0, lvc_ts=384), dict(kp_chunk=1), dict(kp_chunk=2), dict(lvc_pf=0),
           dict(lvc_pf=0, lvc_tpw=1), dict(lvc_pf=1, lvc_tpw=1), dict(lvc_pf=1, lvc_prio=1), dict(lvc_ps=0)]
WN_OPTS = [{}, dict(layer=3), dict(layer=0), dict(layer=0, stack=0), dict(stack=1), dict(stack=4),
           dict(stack=7), dict(stack=10), dict(stack=16), dict(stack=10, stack_ro=16), dict(stack=10, stack_ro=23),
           dict(stack=10, stack_ro=32), dict(stack=10, stack_ro=41), dict(stack=10, stack_ro=44), dict(stack_fuse=0)]
WN_F32_OPTS = [{}, dict(f32_layer=0), dict(f32_layer=2)]
NSF_OPTS = [{}, dict(wconv=0), dict(pair=0), dict(ups_nc=0), dict(rb16=0), dict(rb16=2), dict(rb32=0), dict(rb32=7),
            dict(rb64=7), dict(c256=0, nc_mfma=0), dict(c256=1, nc_mfma=0), dict(c256=0, nc_mfma=2)]


def _name(*parts, **opts):
    return "/".join(parts) + " " + (",".join(f"{k}={v}" for k, v in opts.items()) or "default")


def _tags(run):
    _lib.profile_enable(True)
    try:
        out = run()
        torch.cuda.synchronize()
        assert torch.isfinite(out).all()
        return {t: v[0] for t, v in sorted(_lib.profile_summary().items())}
    finally:
        _lib.profile_enable(False)


def fastdiff_tables():
    """The 4-step sampler (ragged, [3, 2] of 3 frames) and one forward per option set; FD_OPT_LVC_TS 0 takes no
    lens, so that set samples the dense batch."""
    sd = {k: torch.from_numpy(v) for k, v in G.fastdiff_params(31).items()}
    b, a, s, st = fastdiff_infer_params(fastdiff_reverse_schedule(4), fastdiff_train_alpha())
    B, Tc = 2, 3
    mel = torch.from_numpy(synth.synth_inputs(90, (B, Tc, 80), loc=-5.0, scale=2.0)).to(DEV)
    audio = torch.from_numpy(synth.synth_inputs(91, (B, 1, Tc * 256))).to(DEV)
    steps = torch.full((B, 1), 23.47, device=DEV)
    out = {}
    for dtype, sets in (("fp32", [{}]), ("bf16", FD_OPTS)):
        for opts in sets:
            m = FastDiff()
            m.load_state_dict(sd)
            m = m.to(DEV).set_compute_dtype(dtype).set_options(**opts)
            lens = None if opts.get("lvc_ts") == 0 else [3, 2]
            out[_name("fastdiff", dtype, "sample", **opts)] = _tags(
                lambda: m.sample(mel, b, a, s, st, seed=5, lens=lens))
            out[_name("fastdiff", dtype, "forward", **opts)] = _tags(
                lambda: m((audio, mel.transpose(1, 2).contiguous(), steps)))
    return out


def wavenet_tables():
    """The ProDiff denoiser (20 layers, 256 channels): a 2-step ragged sample at T = 70 and a forward at T = 70
    and T = 37 per option set.  Dilation
    cycle 5 at the defaults reaches the stack kernel's dilated instantiations."""
    out = {}
    for cyc, dtype, sets in ((1, "fp32", WN_F32_OPTS), (1, "bf16", WN_OPTS), (5, "bf16", [{}])):
        torch.manual_seed(41)
        sd = GaussianDiffusion(80, WaveNet(80, 256, 20, 256, cyc), timesteps=4, time_scale=1000,
                               max_beta=0.7).state_dict()
        cond = torch.randn(2, 70, 256, device=DEV)
        spec = torch.randn(2, 1, 80, 70, device=DEV)
        steps = torch.tensor([3.0, 1.0], device=DEV)
        for opts in sets:
            g = GaussianDiffusion(80, WaveNet(80, 256, 20, 256, cyc), timesteps=4, time_scale=1000, max_beta=0.7)
            g.load_state_dict(sd)
            g = g.to(DEV).set_compute_dtype(dtype)
            g.denoise_fn.set_options(**opts)
            net = f"wavenet_cyc{cyc}"
            out[_name(net, dtype, "sample", **opts)] = _tags(lambda: g.sample(cond, infer_step=2, seed=7, lens=[70, 41]))
            for T in (70, 37):
                out[_name(net, dtype, f"forward_T{T}", **opts)] = _tags(
                    lambda: g.denoise_fn(spec[..., :T].contiguous(), steps, cond[:, :T].transpose(1, 2).contiguous()))
    return out


def nsf_tables():
    """NSF-HiFiGAN at the SVS dims (512 channels, hop 512), [5, 3] of 5 frames."""
    h = dict(synth.NSF_DEFAULTS)
    sd = {k: torch.from_numpy(v) for k, v in synth.synth_params(synth.nsf_param_shapes(**h), 7).items()}
    rng = np.random.default_rng(8)
    mel = torch.from_numpy(rng.normal(-2.0, 1.0, size=(2, 5, 128)).astype(np.float32)).to(DEV)
    f0 = torch.from_numpy(rng.uniform(60.0, 900.0, size=(2, 5)).astype(np.float32)).to(DEV)
    out = {}
    for dtype, sets in (("fp32", [{}]), ("bf16", NSF_OPTS)):
        for opts in sets:
            g = Generator(h)
            g.load_state_dict(sd)
            g = g.to(DEV).eval().set_compute_dtype(dtype).set_options(**opts)
            out[_name("nsf", dtype, "synthesize", **opts)] = _tags(
                lambda: g.synthesize(mel, f0, 2.30259, seed=9, lens=[5, 3]))
    return out


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("tables", [fastdiff_tables, wavenet_tables, nsf_tables])
def test_dispatch_tags(tables, golden):
    got = tables()
    prefix = next(iter(got)).split("/")[0][:3]
    want = {k: v for k, v in golden.items() if k.startswith(prefix)}
    assert sorted(got) == sorted(want)
    diff = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not diff, diff


if __name__ == "__main__":   # record the fixture (see the module docstring)
    assert "PRODIFF_HIP_LIB" in os.environ, "record with the library of the commit before the change"
    import sys
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    table = {**fastdiff_tables(), **wavenet_tables(), **nsf_tables()}
    with open(path, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{path}: {len(table)} runs")
