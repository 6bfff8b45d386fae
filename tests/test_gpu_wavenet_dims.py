"""The WaveNet denoiser at the dims pd_wavenet_create accepts but the other GPU tests never build.

wavenet_core (prodiff_amd/csrc/wavenet.hip) picks its kernels by M, H, L, C, the dilation cycle and T; every
other test of the denoiser and its samplers runs (H, L, C) = (256, 20, 256).  Each case of tests/wavenet_cases.py
sits on one branch those dims select.  Per case:

  * fp32 against the float64 oracle, max|d| <= 1e-4 (the bar of tests/test_gpu_parity.py);
  * bf16 against the oracle at the shared bar of tests/bf16_bar.py;
  * the launch tags of the run (pd_profile_summary) name the branch the case is for, so a case that silently
    took another path fails instead of passing for the wrong reason;
  * where two bf16 paths compute a frame in the same order (the stack kernel against the one-layer kernel, the
    fused input projection / output stage against the separate launches) their outputs are bit-identical.

Dilation cycles 6 and 7 (dilations 32 and 64) are over the stack window's halo budget (WST_HMAX = 16): they must
take the one-layer kernel.  Before wavenet_core checked that, these nets divided by zero on the host.
"""
import numpy as np
import pytest
import torch

from prodiff_amd import GaussianDiffusion, RectifiedFlow, WaveNet, _lib
from tests import wavenet_cases as WC
from tests.bf16_bar import assert_bf16_close

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-4

FORWARD = list(WC.CASES)
BF16_FORWARD = [n for n in WC.CASES if n not in ("l64", "l65")]   # 64+ layers: no measured bf16 bar, bit-exact checks only
STACK = ["cyc4", "m12", "m132", "l1", "l11"]                      # bf16 forwards that take the stack kernel
PRODIFF = ["cyc4", "cyc6", "wide", "odd", "m12", "m132", "l1"]
REFLOW = ["cyc4", "cyc6", "odd"]
FUSED_TAIL = ["m12", "cyc4"]

# bf16 forward at the default options: tags that must / must not be among the launches
BF16_TAGS = {
    "cyc4": ({"wn_stack"}, {"wn_layer"}),
    "cyc6": ({"wn_layer"}, {"wn_stack"}),
    "cyc7": ({"wn_layer"}, {"wn_stack"}),
    "wide": ({"wn_gate", "wn_resskip"}, {"wn_layer", "wn_stack"}),
    "h192": ({"wn_gate", "wn_resskip"}, {"wn_layer", "wn_stack"}),
    "odd": ({"wn_gate", "wn_resskip"}, {"wn_layer", "wn_stack"}),
    "m12": ({"wn_stack"}, {"wn_inproj", "wn_layer"}),
    "m132": ({"wn_stack", "wn_inproj"}, {"wn_layer"}),
    "m260": ({"wn_layer", "wn_inproj"}, {"wn_stack"}),          # T = 40: below the stack path's 64 frames
    "l1": ({"wn_stack"}, {"wn_layer"}),
    "l11": ({"wn_stack"}, {"wn_layer"}),
    "l11_t63": ({"wn_layer"}, {"wn_stack"}),
}


def tt(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def wavenet(name, dtype, **opts):
    net = WaveNet(*WC.CASES[name]["dims"])
    net.load_state_dict({k: torch.from_numpy(v) for k, v in WC.params(name).items()})
    return net.to(DEV).set_compute_dtype(dtype).set_options(**opts)


def tagged(run):
    """run() twice -- the first call packs the handle -- and the second call's output and launch tags."""
    run()
    torch.cuda.synchronize()
    _lib.profile_enable(True)
    try:
        out = run().float().cpu().numpy()
        tags = set(_lib.profile_summary())
    finally:
        _lib.profile_enable(False)
    return out, tags


def check_tags(tags, want, what):
    has, lacks = want
    print(f"TAGS {what}: {' '.join(sorted(tags))}", flush=True)
    assert has <= tags and not (lacks & tags), (what, sorted(tags))


def assert_close(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = float(np.abs(got - ref).max())
    print(f"F32ERR {what} max|d|={err:.3e} (max|ref| {np.abs(ref).max():.3f})", flush=True)
    assert np.isfinite(got).all() and err <= TOL, f"{what}: max|d|={err:.3e} > {TOL}"


def forward(net, name):
    spec, steps, cond = (tt(a) for a in WC.forward_inputs(name))
    return tagged(lambda: net(spec, steps, cond))


def f32_variants(name):
    _, H, _, C, _ = WC.CASES[name]["dims"]
    return [dict(f32_layer=0), dict(f32_layer=2)] if C == 256 and H == 256 else [{}]


@pytest.mark.parametrize("name,opts", [(n, o) for n in FORWARD for o in f32_variants(n)],
                         ids=lambda v: v if isinstance(v, str) else ",".join(f"{k}={x}" for k, x in v.items()) or "default")
def test_forward_fp32(name, opts):
    """fp32 on the GEMM engine (PD_WN_OPT_F32_LAYER 0, and every net with C or H off 256) and on the direct
    layer kernels (2)."""
    out, tags = forward(wavenet(name, "fp32", **opts), name)
    check_tags(tags, ({"wn_inproj", "wn_gate", "wn_resskip", "wn_skiphead", "wn_outproj"}, {"wn_layer", "wn_stack"}),
               f"{name} fp32 {opts}")
    assert_close(out, WC.forward_ref(name), f"{name} fp32 {opts}")


@pytest.mark.parametrize("name", BF16_FORWARD)
def test_forward_bf16(name):
    """bf16 at the default options: the branch's tags, the shared bf16 bar against the oracle, and for the
    nets on the stack kernel bit-identity with the one-layer kernel (PD_WN_OPT_LAYER 0, PD_WN_OPT_STACK 0)."""
    out, tags = forward(wavenet(name, "bf16"), name)
    check_tags(tags, BF16_TAGS[name], f"{name} bf16")
    if name in STACK:
        one, tags1 = forward(wavenet(name, "bf16", layer=0, stack=0), name)
        check_tags(tags1, ({"wn_layer", "wn_inproj"}, {"wn_stack"}), f"{name} bf16 layer=0,stack=0")
        np.testing.assert_array_equal(out, one)
    assert_bf16_close(out, WC.forward_ref(name), f"{name} forward")


@pytest.mark.parametrize("name,opts,stacked", [("l64", dict(stack=1), True), ("l64", dict(stack=16), True),
                                               ("l65", {}, False)],
                         ids=["l64-stack=1", "l64-stack=16", "l65-default"])
def test_long_stack_bitexact(name, opts, stacked):
    """64 layers are the most the stack path takes (one layer per launch fills its table of 64 groups); 65
    leave it.  Bit-identical to the one-layer kernel either way."""
    out, tags = forward(wavenet(name, "bf16", **opts), name)
    check_tags(tags, ({"wn_stack"}, {"wn_layer"}) if stacked else ({"wn_layer"}, {"wn_stack"}), f"{name} bf16 {opts}")
    one, tags1 = forward(wavenet(name, "bf16", stack=0), name)
    check_tags(tags1, ({"wn_layer"}, {"wn_stack"}), f"{name} bf16 stack=0")
    assert np.isfinite(out).all()
    np.testing.assert_array_equal(out, one)


def prodiff(name, dtype, **opts):
    gd = GaussianDiffusion(WC.CASES[name]["dims"][0], wavenet(name, dtype, **opts), timesteps=WC.PRODIFF_TIMESTEPS,
                           time_scale=1000, max_beta=WC.PRODIFF_MAX_BETA)
    return gd.to(DEV)


def prodiff_sample(gd, name):
    i = WC.sampler_inputs(name)
    cond, xT, nz = tt(i["cond"]), tt(i["x_T"]), tt(i["noise"])
    return tagged(lambda: gd.sample(cond, infer_step=WC.PRODIFF_STEPS, x_T=xT, noise=nz, lens=WC.CASES[name]["lens"]))


def check_sample(name, dtype, out, refs, what):
    got = WC.valid_frames(name, out)
    if dtype == "fp32":
        for k, (g, r) in enumerate(zip(got, refs)):
            assert_close(g, r, f"{what} fp32 run {k}")
    else:
        assert_bf16_close(np.concatenate([g.reshape(-1) for g in got]), np.concatenate([r.reshape(-1) for r in refs]),
                          what)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", PRODIFF)
def test_prodiff_sample(name, dtype):
    """GaussianDiffusion.sample, two steps with explicit draws, ragged where the case has lens: every utterance's
    frames against the oracle's run of that utterance alone.  bf16 with the output stage fused into the last
    stack launch is bit-identical to PD_WN_OPT_STACK_FUSE 0."""
    out, tags = prodiff_sample(prodiff(name, dtype), name)
    print(f"TAGS {name} {dtype} sample: {' '.join(sorted(tags))}", flush=True)
    if dtype == "bf16" and name in FUSED_TAIL:
        assert "wn_stack" in tags and not ({"wn_inproj", "wn_skiphead", "wn_outproj_posterior"} & tags), sorted(tags)
        sep, tags0 = prodiff_sample(prodiff(name, dtype, stack_fuse=0), name)
        check_tags(tags0, ({"wn_stack", "wn_inproj", "wn_skiphead", "wn_outproj_posterior"}, set()),
                   f"{name} bf16 sample stack_fuse=0")
        for a, b in zip(WC.valid_frames(name, out), WC.valid_frames(name, sep)):
            np.testing.assert_array_equal(a, b)
    elif dtype == "bf16":
        assert {"wn_skiphead", "wn_outproj_posterior"} <= tags, sorted(tags)
    check_sample(name, dtype, out, WC.prodiff_ref(name), f"{name} prodiff sample")


@pytest.mark.parametrize("name,tail", [("m12", True), ("m260", False)])
def test_prodiff_sample_f32_tail(name, tail):
    """fp32 with PD_WN_OPT_F32_LAYER 2: the one-launch output stage (wn_f32_tail) holds at most 256 mel bins,
    so M = 260 must leave it for the skip head and the output projection."""
    out, tags = prodiff_sample(prodiff(name, "fp32", f32_layer=2), name)
    check_tags(tags, ({"wn_f32_tail"}, {"wn_skiphead"}) if tail else ({"wn_skiphead", "wn_outproj_posterior"}, {"wn_f32_tail"}),
               f"{name} fp32 sample f32_layer=2")
    check_sample(name, "fp32", out, WC.prodiff_ref(name), f"{name} prodiff sample f32_layer=2")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", REFLOW)
def test_reflow_sample(name, dtype):
    """RectifiedFlow.sample, Euler, three steps (x += v dt fused into the last stack launch where there is one)."""
    i = WC.sampler_inputs(name)
    rf = RectifiedFlow(WC.CASES[name]["dims"][0], wavenet(name, dtype), time_scale=WC.REFLOW_TIME_SCALE,
                       spec_min=[-12], spec_max=[0]).to(DEV)
    cond, xT = tt(i["cond"]), tt(i["x_T_normal"])
    out, tags = tagged(lambda: rf.sample(cond, infer_step=WC.REFLOW_STEPS, x_T=xT, lens=WC.CASES[name]["lens"]))
    print(f"TAGS {name} {dtype} reflow: {' '.join(sorted(tags))}", flush=True)
    if dtype == "bf16" and name == "cyc6":
        assert "wn_layer" in tags and "wn_stack" not in tags, sorted(tags)
    check_sample(name, dtype, out, WC.reflow_ref(name), f"{name} reflow euler")
