"""FD_OPT_LVC_CARRY: the persistent LVC blocks walk runs of consecutive tiles and carry the left halo.

The bf16 4-step FastDiff.sample must be the same bit for bit with the carry (lvc_carry=1), with the
384-row tile walk it replaces (lvc_carry=0) and with the one-tile-per-block kernels (lvc_ps=0).
Small shapes never have more tiles than CUs, so every case caps the persistent grid (lvc_ps_grid):
the runs then hold several tiles of both the final (hop 256) and the hop-64 block.
"""
import numpy as np
import pytest
import torch

from prodiff_amd import FastDiff, _lib, synth
from prodiff_amd.schedules import fastdiff_infer_params, fastdiff_reverse_schedule, fastdiff_train_alpha
from tests import golden_io as G

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def tt(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# B, Tc, lens, grid, draws
#  1 x 12, grid 1: one run from the utterance's first row, 7 carried final tiles (3 072 = 6 x 448 + 384 rows)
#  3 x 23 ragged, grid 4: runs that start mid-utterance, utterance ends inside a carried tile, a partial last
#     tile; explicit draws, and Philox draws keyed by utterance ids
#  2 x 40, grids 5 and 3: unequal run counts per utterance and unequal run lengths
CASES = [(1, 12, None, 1, "explicit"),
         (3, 23, [23, 9, 17], 4, "explicit"),
         (3, 23, [23, 9, 17], 4, "philox_uid"),
         (2, 40, None, 5, "philox"),
         (2, 40, None, 3, "philox")]


@pytest.mark.parametrize("B,Tc,lens,grid,draws", CASES)
def test_fastdiff_lvc_carry_bitexact(B, Tc, lens, grid, draws):
    p = G.fastdiff_params(31)
    b, a, s, st = fastdiff_infer_params(fastdiff_reverse_schedule(4), fastdiff_train_alpha())
    mel = tt(synth.synth_inputs(80 + B, (B, Tc, 80), loc=-5.0, scale=2.0))
    if draws == "explicit":
        kw = dict(x_T=tt(synth.synth_inputs(81 + B, (B, 1, Tc * 256))),
                  noise=tt(synth.synth_inputs(82 + B, (3, B, 1, Tc * 256))))
    elif draws == "philox_uid":
        kw = dict(seed=77, utt_ids=[11, 3, 40][:B])
    else:
        kw = dict(seed=77)
    outs = {}
    for name, opts in (("carry", dict(lvc_carry=1, lvc_ps_grid=grid)), ("walk", dict(lvc_carry=0, lvc_ps_grid=grid)),
                       ("one_tile", dict(lvc_ps=0))):
        m = FastDiff()
        m.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()})
        m = m.to(DEV).set_compute_dtype("bf16").set_options(**opts)
        _lib.profile_enable(True)
        outs[name] = m.sample(mel, b, a, s, st, lens=lens, **kw).cpu().numpy().reshape(B, -1)
        torch.cuda.synchronize()
        prof = _lib.profile_summary()
        _lib.profile_enable(False)
        # both persistent blocks ran (4 steps: 4 launches each)
        assert prof["fd_lvc_block_final"][0] == 4 and prof["fd_lvc_block_ups"][0] >= 4, prof
    assert np.isfinite(outs["carry"]).all()
    for r in range(B):
        n = (lens[r] if lens else Tc) * 256
        np.testing.assert_array_equal(outs["carry"][r, :n], outs["one_tile"][r, :n])
        np.testing.assert_array_equal(outs["walk"][r, :n], outs["one_tile"][r, :n])
