"""The FFT-block encoders at the dims pd_cond_create, pd_pitch_cond_create and pd_dur_create accept but the other
GPU tests never build.

fft_stack_forward (prodiff_amd/csrc/encoder.hip, fft_stack.h) picks its attention kernel by the head dim, its
GEMM tile per GEMM by the row count and N (enc_gemm), and its create walk by the handle's flags; every other test
runs hidden_size 256, FFN kernel 9 and at most 600 rows.  Each case of tests/encoder_cases.py sits on one branch
those dims select (tests/test_encoder_dims_cpu.py pins which).  Per case:

  * fp32 against the float64 oracle, max|d| <= 1e-4 (the bar of tests/test_gpu_cond.py and test_gpu_variance.py),
    durations within 1e-4 * max(1, |ref|), exact zeros on padding; two calls are bit-identical;
  * bf16 against the oracle at the shared bar of tests/bf16_bar.py;
  * ragged cases: each row of the padded batch, given its lengths, equals the row encoded alone within
    1e-5 * max|alone| (the bound of tests/test_gpu_variance.py);
  * through the C ABI with exactly pd_*_workspace_size bytes carved from a larger buffer: the bytes after the
    workspace and after every output keep their pattern, in fp32 and in bf16, and the outputs are the module's;
    that size is the one tests/encoder_cases.py restates from the tile choice, which ties the restatement (and
    with it the branch each case claims) to the library's own enc_ksplit.

The RelPositionalEncoding table is grown by a real 5,003-token batch going through the module, not by hand; the
same batch through a handle packed for a 5,000-row table runs the embedding kernel's T_txt > table arm.

No case exposed a bug: every one passes its bars with the kernels as they were, so nothing was fixed and no
accepted shape became a rejection (the measured errors: profiles/encoder_dims/gpu_tests.log).
"""
import functools

import numpy as np
import pytest
import torch

from prodiff_amd import _lib
from tests import encoder_cases as EC
from tests import variance_cases as VC
from tests.bf16_bar import assert_bf16_close

pytestmark = pytest.mark.gpu
TOL = 1e-4
RAGGED_REL = 1e-5
GUARD = 1 << 20          # bytes of pattern after every buffer of a C-ABI call
PATTERN = 0xA5

COND = list(EC.COND_CASES)
PITCH = list(EC.PITCH_CASES)
DUR = list(EC.DUR_CASES)
# every case is in both lists: none missed the shared bf16 bar
BF16_COND, BF16_PITCH, BF16_DUR = COND, PITCH, DUR
BOUNDS = [("cond", "h192_d64"), ("cond", "k11"), ("cond", "rows2000"), ("cond", "rows8096"), ("pitch", "note64"),
          ("dur", "c32_k11"), ("dur", "dur_rows8096")]


def cuda(ins):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in ins.items()}


def _load(m, P):
    missing, unexpected = m.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()}, strict=False)
    assert not unexpected
    assert all(k.startswith("diffusion.") or k.endswith("_float_tensor") for k in missing), missing
    return m.cuda()


def model(family, name, dtype="fp32"):
    from prodiff_amd import DurPredictor, PitchPredictor
    from prodiff_amd.teacher import ProDiffTeacher
    hp = EC.hp_of(family, name)
    if family == "cond":
        m = ProDiffTeacher(EC.VOCAB, EC.teacher_hparams(hp))
    elif family == "pitch":
        m = PitchPredictor(EC.VOCAB, VC.reference_pitch_hparams(hp))
    else:
        m = DurPredictor(EC.VOCAB, VC.reference_dur_hparams(hp))
    return _load(m, EC.params(family, name)).set_compute_dtype(dtype)


def cond_forward(t, name, ins=None, lens=None):
    """(cond, enc) of the case's batch (or ``ins``), with the rows' phoneme counts where the case gives them."""
    x = cuda(EC.inputs("cond", name) if ins is None else ins)
    if lens is None and ins is None and EC.case("cond", name).get("txt_lens"):
        lens = EC.case("cond", name)["lengths"]
    return t.forward_condition(x.pop("txt_tokens"), x.pop("mel2ph"), x.pop("f0"), return_encoder=True, txt_lens=lens, **x)


def dur_forward(m, name, ins=None, lens=None):
    return m(**cuda(EC.inputs("dur", name) if ins is None else ins), return_log=True, txt_lens=lens)


def _pieces(v):
    return v if isinstance(v, list) else [v]


def assert_close(got, ref, what):
    """fp32: every piece (the batch, or each row of a txt_lens batch) within TOL of the oracle."""
    err, top = 0.0, 0.0
    for g, r in zip(_pieces(got), _pieces(ref)):
        g, r = np.asarray(g, np.float64), np.asarray(r, np.float64)
        assert g.shape == r.shape, (what, g.shape, r.shape)
        assert np.isfinite(g).all(), what
        err, top = max(err, float(np.abs(g - r).max())), max(top, float(np.abs(r).max()))
    print(f"F32ERR {what} max|d|={err:.3e} (max|ref| {top:.3f})", flush=True)
    assert err <= TOL, f"{what}: max|d|={err:.3e} > {TOL}"


def assert_low_close(got, ref, what):
    flat = lambda v: np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in _pieces(v)])
    assert_bf16_close(flat(got), flat(ref), what)


def check_cond(name, dtype, cond, enc, again):
    ins = EC.inputs("cond", name)
    assert torch.equal(cond, again[0]) and torch.equal(enc, again[1]), "two calls differ"
    cond, enc = cond.cpu().numpy(), enc.cpu().numpy()
    assert np.all(cond[ins["mel2ph"] == 0] == 0) and np.all(enc[ins["txt_tokens"] == 0] == 0)
    got_c, got_e = EC.cond_valid(name, cond, enc)
    ref_c, ref_e = EC.cond_ref(name)
    if dtype == "fp32":
        assert_close(got_e, ref_e, f"cond {name} enc")
        assert_close(got_c, ref_c, f"cond {name} cond")
    else:
        assert_low_close(got_e, ref_e, f"cond {name} enc")
        assert_low_close(got_c, ref_c, f"cond {name} cond")


# ---------------------------------------------------------------- parity
@pytest.mark.parametrize("name", COND)
def test_cond_fp32(name):
    t = model("cond", name)
    check_cond(name, "fp32", *cond_forward(t, name), cond_forward(t, name))


@pytest.mark.parametrize("name", BF16_COND)
def test_cond_bf16(name):
    t = model("cond", name, "bf16")
    check_cond(name, "bf16", *cond_forward(t, name), cond_forward(t, name))


@pytest.mark.parametrize("name", PITCH)
def test_pitch_cond_fp32(name):
    m, x = model("pitch", name), cuda(EC.inputs("pitch", name))
    cond = m.forward_condition(**x)
    assert torch.equal(cond, m.forward_condition(**x)), "two calls differ"
    assert_close(cond.cpu().numpy(), EC.pitch_ref(name), f"pitch {name} cond")


@pytest.mark.parametrize("name", BF16_PITCH)
def test_pitch_cond_bf16(name):
    m, x = model("pitch", name, "bf16"), cuda(EC.inputs("pitch", name))
    cond = m.forward_condition(**x)
    assert torch.equal(cond, m.forward_condition(**x)), "two calls differ"
    assert_low_close(cond.cpu().numpy(), EC.pitch_ref(name), f"pitch {name} cond")


@pytest.mark.parametrize("name", DUR)
def test_dur_fp32(name):
    m = model("dur", name)
    dur, log = dur_forward(m, name)
    again = dur_forward(m, name)
    assert torch.equal(dur, again[0]) and torch.equal(log, again[1]), "two calls differ"
    dur, log = dur.cpu().numpy(), log.cpu().numpy()
    ref_dur, ref_log = EC.dur_ref(name)
    assert_close(log, ref_log, f"dur {name} log")
    e_dur = float((np.abs(dur - ref_dur) / np.maximum(1.0, np.abs(ref_dur))).max())
    print(f"F32ERR dur {name} dur max rel|d|={e_dur:.3e} (max|ref| {ref_dur.max():.3f})", flush=True)
    assert np.isfinite(dur).all() and e_dur <= TOL
    pad = EC.inputs("dur", name)["txt_tokens"] == 0
    assert np.all(dur[pad] == 0) and np.all(log[pad] == 0)


@pytest.mark.parametrize("name", BF16_DUR)
def test_dur_bf16(name):
    m = model("dur", name, "bf16")
    _, log = dur_forward(m, name)
    assert torch.equal(log, dur_forward(m, name)[1]), "two calls differ"
    assert_low_close(log.cpu().numpy(), EC.dur_ref(name)[1], f"dur {name} log")


# ---------------------------------------------------------------- ragged rows
def _ragged(what, batch_row, alone):
    err = float((batch_row - alone).abs().max())
    bound = RAGGED_REL * float(alone.abs().max())
    print(f"RAGGED {what} max|d|={err:.3e} bound={bound:.3e}", flush=True)
    assert err <= bound, (what, err, bound)


@pytest.mark.parametrize("name", ["k11", "rows2000"])
def test_cond_ragged_rows_equal_alone(name):
    """Each row of the padded batch, given txt_lens, equals the row encoded alone -- across the GEMM tiles: the
    2000-row batch runs its FFN conv on the 128 x 64 tile, a row alone on split-K tiles."""
    t, ins = model("cond", name), EC.inputs("cond", name)
    cond, enc = cond_forward(t, name)
    for b, n in enumerate(EC.case("cond", name)["lengths"]):
        c1, e1 = cond_forward(t, name, ins=EC.cond_row_alone(ins, b, n))
        _ragged(f"cond {name} row {b} enc", enc[b, :n], e1[0])
        _ragged(f"cond {name} row {b} cond", cond[b, :c1.shape[1]], c1[0])


def test_pitch_ragged_rows_equal_alone():
    name = "note64"
    m, ins = model("pitch", name), EC.inputs("pitch", name)
    tl, nl = EC.lens_of("pitch", name)
    cond = m.forward_condition(**cuda(ins), txt_lens=tl, note_lens=nl)
    for b in range(len(tl)):
        alone = m.forward_condition(**cuda(VC.row_alone(ins, b, tl[b], nl[b])))[0]
        _ragged(f"pitch {name} row {b}", cond[b, :alone.shape[0]], alone)


def test_dur_ragged_rows_equal_alone():
    name = "c32_k11"
    m, ins = model("dur", name), EC.inputs("dur", name)
    tl, _ = EC.lens_of("dur", name)
    _, log = dur_forward(m, name, lens=tl)
    for b in range(len(tl)):
        _, alone = dur_forward(m, name, ins=VC.row_alone(ins, b, tl[b]))
        _ragged(f"dur {name} row {b}", log[b, :tl[b]], alone[0])


# ---------------------------------------------------------------- workspace and output bounds
def _guarded(nbytes):
    """nbytes of buffer followed by GUARD bytes, all holding the pattern."""
    return torch.full((int(nbytes) + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")


def _intact(buf, nbytes):
    return bool((buf[int(nbytes):] == PATTERN).all())


def _floats(buf, shape):
    return buf[:4 * int(np.prod(shape))].view(torch.float32).reshape(shape)


def _vp(t):
    return None if t is None else _lib.C.c_void_p(t.data_ptr())


def cond_cabi(t, name, lens=None):
    """pd_cond_forward on the module's handle with exactly pd_cond_workspace_size bytes -> (cond, enc); the
    bytes after the workspace and after both outputs must keep their pattern."""
    L, h, x = _lib.lib(), t.cond_handle(), cuda(EC.inputs("cond", name))
    B, Tt = x["txt_tokens"].shape
    Tm, H = x["mel2ph"].shape[1], t.encoder.hidden_size
    tl = _lib.lens(lens, B, Tt, x["txt_tokens"].device)
    g = lambda k: _vp(x.get(k))
    ins = _lib.pd_cond_inputs(g("txt_tokens"), g("mel2ph"), g("f0"), g("lang_seq"), g("spk_embed_id"), None, 0, None,
                              None, 0, g("voicing"), g("breath"), _vp(tl))
    nb = L.pd_cond_workspace_size(h, B, Tt, Tm)
    assert nb == EC.workspace_bytes("cond", name), "the library's tile choice is not the restated one"
    ws, cond, enc = _guarded(nb), _guarded(4 * B * Tm * H), _guarded(4 * B * Tt * H)
    _lib.check(L.pd_cond_forward(h, _lib.C.byref(ins), _vp(cond), _vp(enc), B, Tt, Tm, _vp(ws), nb, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert _intact(ws, nb), "wrote past the workspace"
    assert _intact(cond, 4 * B * Tm * H) and _intact(enc, 4 * B * Tt * H), "wrote past an output"
    assert L.pd_cond_forward(h, _lib.C.byref(ins), _vp(cond), _vp(enc), B, Tt, Tm, _vp(ws), nb - 1,
                             _lib.stream_ptr()) == 3                      # PD_ERR_WORKSPACE: the size is exact
    return _floats(cond, (B, Tm, H)), _floats(enc, (B, Tt, H))


def pitch_cabi(m, name, tl, nl):
    L, h, x = _lib.lib(), m.cond_handle(), cuda(EC.inputs("pitch", name))
    B, Tt = x["txt_tokens"].shape
    Tn, Tm, H = x["note_midi"].shape[1], x["mel2ph"].shape[1], m.encoder.hidden_size
    dev = x["txt_tokens"].device
    rest = (x["note_rest"] != 0).to(torch.uint8).contiguous()
    tl, nl = _lib.lens(tl, B, Tt, dev), _lib.lens(nl, B, Tn, dev)
    ins = _lib.pd_pitch_cond_inputs(_vp(x["txt_tokens"]), _vp(x["mel2ph"]), _vp(x["note_midi"]), _vp(rest),
                                    _vp(x["mel2note"]), _vp(x.get("spk_id")), _vp(x["pitch_expr"].reshape(B).contiguous()),
                                    None, None, None, _vp(tl), _vp(nl))
    nb = L.pd_pitch_cond_workspace_size(h, B, Tt, Tn, Tm)
    assert nb == EC.workspace_bytes("pitch", name), "the library's tile choice is not the restated one"
    ws, cond = _guarded(nb), _guarded(4 * B * Tm * H)
    _lib.check(L.pd_pitch_cond_forward(h, _lib.C.byref(ins), _vp(cond), B, Tt, Tn, Tm, _vp(ws), nb, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert _intact(ws, nb), "wrote past the workspace"
    assert _intact(cond, 4 * B * Tm * H), "wrote past the output"
    return _floats(cond, (B, Tm, H))


def dur_cabi(m, name, tl):
    L, h, x = _lib.lib(), m.dur_handle(), cuda(EC.inputs("dur", name))
    B, Tt = x["txt_tokens"].shape
    tl = _lib.lens(tl, B, Tt, x["txt_tokens"].device)
    ins = _lib.pd_dur_inputs(_vp(x["txt_tokens"]), _vp(x["onset"]), _vp(x["word_dur"]), _vp(tl))
    nb = L.pd_dur_workspace_size(h, B, Tt)
    assert nb == EC.workspace_bytes("dur", name), "the library's tile choice is not the restated one"
    ws, log, dur = _guarded(nb), _guarded(4 * B * Tt), _guarded(4 * B * Tt)
    _lib.check(L.pd_dur_forward(h, _lib.C.byref(ins), _vp(log), _vp(dur), B, Tt, _vp(ws), nb, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert _intact(ws, nb), "wrote past the workspace"
    assert _intact(log, 4 * B * Tt) and _intact(dur, 4 * B * Tt), "wrote past an output"
    return _floats(dur, (B, Tt)), _floats(log, (B, Tt))


@pytest.mark.parametrize("family,name", BOUNDS, ids=[f"{f}-{n}" for f, n in BOUNDS])
def test_workspace_and_output_bounds(family, name):
    """fp32, then bf16 (the handle is packed again): nothing is written outside the exact-size workspace and the
    outputs, with the rows' lengths given, and the C-ABI call computes what the module's call does."""
    m = model(family, name)
    tl, nl = EC.lens_of(family, name)
    for dtype in ("fp32", "bf16"):
        m.set_compute_dtype(dtype)
        if family == "cond":
            got = cond_cabi(m, name, tl)
            want = cond_forward(m, name, lens=tl)
        elif family == "pitch":
            got = (pitch_cabi(m, name, tl, nl),)
            want = (m.forward_condition(**cuda(EC.inputs("pitch", name)), txt_lens=tl, note_lens=nl),)
        else:
            got = dur_cabi(m, name, tl)
            want = dur_forward(m, name, lens=tl)
        for g, w in zip(got, want):
            assert torch.isfinite(g).all() and torch.equal(g, w), (family, name, dtype)


# ---------------------------------------------------------------- a rel-pos table that a real batch grew
@functools.lru_cache(maxsize=None)
def _relpos_refs():
    return EC.cond_ref("relpos_over_table"), EC.cond_ref("relpos_after")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_relpos_over_table(dtype):
    """A B = 1 batch of 5,003 tokens: first through the C ABI on the handle packed for the 5,000-row table
    (enc_embed_kernel's T_txt > table arm), then through the module, which grows its table to 5,003 rows first --
    the same positions, so bit-identical.  Then the short batch through the same module with no manual
    extend: its reversed positions count from 5,003, as the reference's table after that batch."""
    (ref_c, ref_e), (aft_c, aft_e) = _relpos_refs()
    t = model("cond", "relpos_over_table", dtype)
    pos = t.encoder.embed_positions
    assert pos.pe_len == 5000
    low_c, low_e = cond_cabi(t, "relpos_over_table")
    assert pos.pe_len == 5000 and t.cond_dims().rel_pos == 5000
    cond, enc = cond_forward(t, "relpos_over_table")
    assert pos.pe_len == EC.RELPOS_LONG and t.cond_dims().rel_pos == EC.RELPOS_LONG
    assert torch.equal(cond, low_c) and torch.equal(enc, low_e)
    short_c, short_e = cond_forward(t, "relpos_after")
    assert pos.pe_len == EC.RELPOS_LONG
    close = assert_close if dtype == "fp32" else assert_low_close
    close(enc.cpu().numpy(), ref_e, f"cond relpos_over_table enc {dtype}")
    close(cond.cpu().numpy(), ref_c, f"cond relpos_over_table cond {dtype}")
    close(short_e.cpu().numpy(), aft_e, f"cond relpos_after enc {dtype}")
    close(short_c.cpu().numpy(), aft_c, f"cond relpos_after cond {dtype}")
    # the short batch on a fresh module (a 5,000-row table) is another encoding: the growth is what is tested
    fresh = cond_forward(model("cond", "relpos_after", dtype), "relpos_after")[1]
    assert float((fresh - short_e).abs().max()) > 1e-2
