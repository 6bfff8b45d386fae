"""WaveNet denoiser configurations away from the ProDiff default (M, H, L, C) = (80, 256, 20, 256), one per
branch of wavenet_core (prodiff_amd/csrc/wavenet.hip) that the dims select, with synthetic weights and inputs
and the float64 oracle's outputs (oracle/oracle_prodiff.py, oracle/oracle_reflow.py) for them.

Nothing here needs a GPU.  The oracle outputs are computed once per process and case (lru_cache) and shared by
every dtype and option variant of tests/test_gpu_wavenet_dims.py; callers must not modify the arrays.

A case with `lens` is a ragged batch for the samplers: the oracle runs each row alone (B = 1, T = lens[b]),
which is what a padded batch has to equal on that row's first lens[b] frames (include/prodiff_hip.h).
"""
from functools import lru_cache

import numpy as np

from oracle import oracle_prodiff as OP
from oracle import oracle_reflow as OR
from prodiff_amd import synth

# name: (M, H, L, C, cyc), B, T, lens -- and the branch the case is for
CASES = {
    # stack groups {1,2,4,8} x 5 (DiffSinger's usual cycle)
    "cyc4": dict(dims=(80, 256, 20, 256, 4), B=2, T=70, lens=[70, 41]),
    # dilation 32 is over the stack window's halo budget: the one-layer kernel
    "cyc6": dict(dims=(80, 256, 12, 256, 6), B=2, T=70, lens=[70, 41]),
    # dilation 64 with both taps inside the utterance
    "cyc7": dict(dims=(64, 256, 8, 256, 7), B=1, T=130, lens=None),
    # C != 256: the GEMM engine in both dtypes, split K
    "wide": dict(dims=(80, 256, 4, 512, 1), B=2, T=37, lens=None),
    # C = 256 but 3C + H != 1024: no fragment weights, no fp32 direct kernel
    "h192": dict(dims=(80, 192, 4, 256, 2), B=2, T=37, lens=None),
    # H no multiple of 32 (padded K segment), C no multiple of 64, M < 32, T < 32
    "odd": dict(dims=(12, 36, 3, 96, 3), B=3, T=29, lens=None),
    # fused input projection and fused tail with M below one wave's 32 columns
    "m12": dict(dims=(12, 256, 12, 256, 1), B=2, T=70, lens=None),
    # packed W_in rows longer than 128: the stack with the separate input projection, tail unfused
    "m132": dict(dims=(132, 256, 12, 256, 1), B=2, T=70, lens=None),
    # M > 256: the fp32 tail kernel does not take it
    "m260": dict(dims=(260, 256, 4, 256, 1), B=1, T=40, lens=None),
    # first == last layer; one stack group, so no fused tail
    "l1": dict(dims=(80, 256, 1, 256, 1), B=2, T=70, lens=None),
    # groups 10 + 1 at the smallest T the stack path takes, and one frame below it
    "l11": dict(dims=(80, 256, 11, 256, 1), B=2, T=64, lens=None),
    "l11_t63": dict(dims=(80, 256, 11, 256, 1), B=2, T=63, lens=None),
    # 64 groups of one layer fill the group table; 65 layers leave the stack
    "l64": dict(dims=(80, 256, 64, 256, 1), B=1, T=64, lens=None),
    "l65": dict(dims=(80, 256, 65, 256, 1), B=1, T=64, lens=None),
}
PRODIFF_STEPS, PRODIFF_TIMESTEPS, PRODIFF_MAX_BETA = 2, 2, 40.0
REFLOW_STEPS, REFLOW_TIME_SCALE = 3, 1000


def _seed(name):
    return 1000 + 10 * list(CASES).index(name)


@lru_cache(maxsize=None)
def params(name):
    """The reference state dict, every parameter drawn (the module zero-initialises output_projection)."""
    M, H, L, C, _ = CASES[name]["dims"]
    return synth.synth_params(synth.wavenet_param_shapes(M, H, L, C), _seed(name))


@lru_cache(maxsize=None)
def forward_inputs(name):
    """spec [B,1,M,T], steps [B] (distinct, non-integer), cond [B,H,T]."""
    c = CASES[name]
    M, H = c["dims"][:2]
    s = _seed(name)
    spec = synth.synth_inputs(s + 1, (c["B"], 1, M, c["T"]))
    cond = synth.synth_inputs(s + 2, (c["B"], H, c["T"]))
    steps = (3.25 + 117.5 * np.arange(c["B"])).astype(np.float32)
    return spec, steps, cond


@lru_cache(maxsize=None)
def forward_ref(name):
    L, cyc = CASES[name]["dims"][2], CASES[name]["dims"][4]
    return OP.wavenet_forward(params(name), *forward_inputs(name), L, cyc)


@lru_cache(maxsize=None)
def sampler_inputs(name):
    """cond [B,T,H], x_T [B,1,M,T] uniform (ProDiff) and normal (rectified flow), noise [S,B,1,M,T]."""
    c = CASES[name]
    M, H = c["dims"][:2]
    s = _seed(name)
    return dict(cond=synth.synth_inputs(s + 3, (c["B"], c["T"], H)),
                x_T=synth.synth_inputs(s + 4, (c["B"], 1, M, c["T"]), kind="uniform"),
                noise=synth.synth_inputs(s + 5, (PRODIFF_STEPS, c["B"], 1, M, c["T"])),
                x_T_normal=synth.synth_inputs(s + 6, (c["B"], 1, M, c["T"])))


def _rows(name):
    """(row, frames) of the runs the oracle makes: the whole batch (row None), or each utterance alone."""
    c = CASES[name]
    return [(None, c["T"])] if c["lens"] is None else list(enumerate(c["lens"]))


def valid_frames(name, out):
    """A sampler's [B,T,M] output as the list of arrays the *_ref functions return."""
    return [out if b is None else out[b, :n] for b, n in _rows(name)]


@lru_cache(maxsize=None)
def prodiff_ref(name):
    """GaussianDiffusion.sample, PRODIFF_STEPS steps with the explicit draws: the dense batch's mel [B,T,M], or
    each row's mel [lens[b], M] from its own run."""
    L, cyc = CASES[name]["dims"][2], CASES[name]["dims"][4]
    bufs = OP.diffusion_buffers(OP.vpsde_betas(PRODIFF_TIMESTEPS, PRODIFF_MAX_BETA))
    bufs["timesteps"] = PRODIFF_TIMESTEPS
    i = sampler_inputs(name)
    out = []
    for b, n in _rows(name):
        r = slice(None) if b is None else slice(b, b + 1)
        mel = OP.prodiff_sample(params(name), bufs, i["cond"][r, :n], i["x_T"][r, ..., :n], i["noise"][:, r, ..., :n],
                                L, cyc, PRODIFF_STEPS)
        out.append(mel if b is None else mel[0])
    return out


@lru_cache(maxsize=None)
def reflow_ref(name):
    """RectifiedFlow.sample, Euler, REFLOW_STEPS steps from x_T_normal; rows as prodiff_ref."""
    L, cyc = CASES[name]["dims"][2], CASES[name]["dims"][4]
    i = sampler_inputs(name)
    out = []
    for b, n in _rows(name):
        r = slice(None) if b is None else slice(b, b + 1)
        x = OR.reflow_sample(params(name), i["cond"][r, :n], i["x_T_normal"][r, ..., :n], REFLOW_STEPS, "euler",
                             REFLOW_TIME_SCALE, L, cyc)
        out.append(x if b is None else x[0])
    return out
