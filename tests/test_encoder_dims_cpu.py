"""CPU side of the FFT-block encoders' accepted dims (tests/encoder_cases.py, tests/test_gpu_encoder_dims.py):

  * every case sits on the branch it is for -- the GEMM tile that enc_gemm (fft_stack.h:95-116) picks for each of
    its GEMMs, the key chunks of its attention, the column masking -- so a later change of lengths cannot drop
    a case off its branch unnoticed, and the tile switch sits at the row counts the kernels' header states;
  * the float64 oracles (oracle/oracle_encoder.py, tests/variance_ref.py) reproduce the reference modules' own
    outputs at the new dims (tests/golden/encdims_*.npz) within the bound tests/test_oracle.py and
    tests/test_variance_cpu.py use;
  * the three creates reject the dims the kernels do not take, with an error text, before they touch a device
    (this machine has none, so a create that launched anything would fail differently).
"""
import numpy as np
import pytest

from oracle import oracle_encoder as OE
from prodiff_amd import _lib
from tests import encoder_cases as EC

ORACLE_TOL = 5e-5   # tests/test_oracle.py's bound for the cond_* fixtures: the fp32 reference's own rounding
ALL = [(f, n) for f in EC.FAMILIES for n in EC.FAMILIES[f]]


# ---------------------------------------------------------------- (a) the branch of every case
@pytest.mark.parametrize("family,name", ALL, ids=[f"{f}-{n}" for f, n in ALL])
def test_case_takes_its_tiles(family, name):
    """The GEMMs a case names under ``big`` take the 128 x 64 tile and no other GEMM of it does."""
    t = EC.tiles(family, name)
    big = {g for g, v in t.items() if v == "big"}
    assert big == set(EC.case(family, name).get("big", ())), (name, t)
    assert all(v == "big" or 1 <= v <= 8 for v in t.values())


def test_tile_boundaries():
    """enc_big_tile flips where fft_stack.h says: the FFN conv of H = 256 (N = 1024) between 1920 and 1921
    rows, out-proj and FFN-2 (N = 256) between 8064 and 8065, QKV (N = 768) between 2688 and 2689, the
    duration predictor's convs at n_chans = 512 between 3968 and 3969."""
    for N, last in ((1024, 1920), (256, 8064), (768, 2688), (512, 3968)):
        assert not EC.enc_big_tile(last, N) and EC.enc_big_tile(last + 1, N), (N, last)
        assert EC.enc_ksplit(last + 1, N, 256) == 1
    # split-K: at most 8 blocks, at least 4 K steps each, none below 8 K steps (K = 64: note_encode_out_linear)
    assert EC.enc_ksplit(31, 768, 256) == 2 and EC.enc_ksplit(31, 1024, 9 * 256) == 8
    assert EC.enc_ksplit(31, 128, 64) == 1 and EC.enc_ksplit(600, 1024, 9 * 256) == 2


def test_cases_reach_their_branches():
    chunks = {n: EC.key_chunks("cond", n) for n in EC.COND_CASES}
    assert chunks["h64_d64"] == 2 and min(EC.COND_CASES["h64_d64"]["lengths"]) < EC.AK    # the online-softmax carry
    assert chunks["h128_d64"] == 3
    assert chunks["t1"] == 1 and EC.inputs("cond", "t1")["mel2ph"].sum(1).tolist() == [1, 2, 3]
    for n in ("h64_d64", "h128_d64", "h192_d64", "h320_d64"):
        hp = EC.hp_of("cond", n)
        assert hp["hidden_size"] // hp["num_heads"] == 64
    assert EC.hp_of("cond", "h512_d256")["hidden_size"] // EC.hp_of("cond", "h512_d256")["num_heads"] == 256
    assert EC.hp_of("cond", "h512_d128")["hidden_size"] // EC.hp_of("cond", "h512_d128")["num_heads"] == 128
    g = EC.gemms("cond", "h192_d64")
    assert g["qkv"][1] % 128 and g["ffn1"][1] % 128 == 0 and g["outproj"][1] % 128     # 576, 768, 192 columns
    # k = 11: the five right-hand taps cross every row's own end inside the padded batch
    c = EC.COND_CASES["k11"]
    assert c["pad_tokens"] >= 11 // 2 + 1 and c["txt_lens"] and EC.hp_of("cond", "k11")["enc_ffn_kernel_size"] == 11
    # ragged rows everywhere, padding everywhere but the one-token case
    for fam, n in ALL:
        c = EC.case(fam, n)
        assert c["pad_tokens"] >= 1 or n in ("t1", "tn1", "relpos_over_table"), n
    assert EC.inputs("cond", "rows2000")["txt_tokens"].shape == (8, 250)
    assert EC.inputs("cond", "rows8096")["txt_tokens"].shape == (32, 253)
    assert EC.inputs("dur", "dur_rows8096")["txt_tokens"].shape == (32, 253)
    assert EC.inputs("cond", "relpos_over_table")["txt_tokens"].shape == (1, EC.RELPOS_LONG) and EC.RELPOS_LONG > 5000
    # note_encode_out_linear with K = 64: two K steps and no split
    assert EC.gemms("pitch", "note64")["note_out"][2] == 2 * EC.GEMM_BK and EC.tiles("pitch", "note64")["note_out"] == 1
    assert EC.inputs("pitch", "tn1")["txt_tokens"].shape[1] == 1 and EC.inputs("pitch", "tn1")["note_midi"].shape[1] == 1
    assert "spk_id" not in EC.inputs("pitch", "nospk")
    assert set(EC.inputs("cond", "flags_min")) == {"txt_tokens", "mel2ph", "f0"}
    assert "breath" in EC.inputs("cond", "breath_only") and "voicing" not in EC.inputs("cond", "breath_only")


# ---------------------------------------------------------------- (b) the oracles at the new dims
@pytest.mark.parametrize("name", EC.fixture_cases("cond"))
def test_cond_oracle_matches_reference(name):
    d = EC.fixture("cond", name)
    x = EC.inputs("cond", name)
    assert all(np.array_equal(d[k], v) for k, v in x.items()), "the stored inputs are not what synth draws"
    cond, enc = OE.forward_condition(EC.params("cond", name), EC.hp_of("cond", name), return_encoder=True, **x)
    e1, e2 = float(np.abs(enc - d["enc"]).max()), float(np.abs(cond - d["cond"]).max())
    print(f"CONDREF {name} enc max|d|={e1:.3e} cond max|d|={e2:.3e} max|cond|={np.abs(d['cond']).max():.3f}", flush=True)
    assert e1 <= ORACLE_TOL and e2 <= ORACLE_TOL
    assert np.all(cond[x["mel2ph"] == 0] == 0)


@pytest.mark.parametrize("name", EC.fixture_cases("pitch"))
def test_pitch_oracle_matches_reference(name):
    d = EC.fixture("pitch", name)
    x = EC.inputs("pitch", name)
    assert all(np.array_equal(d[k], v) for k, v in x.items())
    assert [str(k) for k in d["state_dict_keys"] if not str(k).startswith("diffusion.")
            and not str(k).endswith("_float_tensor")] == list(EC.params("pitch", name))
    err = float(np.abs(EC.pitch_ref(name) - d["cond"]).max())
    print(f"PITCHREF {name} max|d|={err:.3e} max|cond|={np.abs(d['cond']).max():.3f}", flush=True)
    assert err <= ORACLE_TOL


@pytest.mark.parametrize("name", EC.fixture_cases("dur"))
def test_dur_oracle_matches_reference(name):
    d = EC.fixture("dur", name)
    x = EC.inputs("dur", name)
    assert all(np.array_equal(d[k], v) for k, v in x.items())
    dur, log = EC.dur_ref(name)
    e_log = float(np.abs(log - d["log"]).max())
    e_dur = float((np.abs(dur - d["dur"]) / np.maximum(1.0, np.abs(d["dur"]))).max())
    print(f"DURREF {name} log max|d|={e_log:.3e} dur rel={e_dur:.3e}", flush=True)
    assert e_log <= ORACLE_TOL and e_dur <= ORACLE_TOL
    nonpad = x["txt_tokens"] != 0
    assert np.all(d["dur"][~nonpad] == 0) and np.all(d["log"][~nonpad] == 0)
    assert 2 * int((d["dur"][nonpad] > 0).sum()) >= int(nonpad.sum())   # the clamp does not hide the head


def test_row_count_cases_keep_the_head_visible():
    dur, _ = EC.dur_ref("dur_rows8096")
    nonpad = EC.inputs("dur", "dur_rows8096")["txt_tokens"] != 0
    assert 2 * int((dur[nonpad] > 0).sum()) >= int(nonpad.sum())


@pytest.mark.parametrize("name", ["k11", "rows2000"])
def test_row_alone_oracle_differs_from_the_padded_batch(name):
    """With txt_lens the oracle of the rows alone is not the padded batch's, by far more than the fp32 bar
    (else the case would not tell whether the kernels read lens on the tile its FFN conv takes)."""
    x, P, hp = EC.inputs("cond", name), EC.params("cond", name), EC.hp_of("cond", name)
    _, enc = OE.forward_condition(P, hp, return_encoder=True, **x)
    _, alone = EC.cond_ref(name)
    for b, n in enumerate(EC.COND_CASES[name]["lengths"]):
        assert np.abs(enc[b, :n] - alone[b]).max() > 1e-3, b


# ---------------------------------------------------------------- (c) dims the creates refuse
ARG, UNSUPPORTED = 1, 4   # PD_ERR_ARG, PD_ERR_UNSUPPORTED (include/prodiff_hip.h)


def _create(fn, dims, n):
    """create with a parameter list of n null pointers: a create that got past its dims checks reports the
    first null parameter, so the error text tells a rejected dim from accepted ones."""
    lib = _lib.lib()
    h = _lib.C.c_void_p()
    params = (_lib.C.c_void_p * max(n, 1))()
    rc = getattr(lib, fn)(_lib.C.byref(dims), params, 0, None, _lib.C.byref(h))
    assert h.value is None
    return rc, lib.pd_last_error().decode()


def cond(H=256, L=1, k=9, heads=2, rel_pos=0):
    return _create("pd_cond_create", _lib.pd_cond_dims(40, H, L, k, heads, 1, 3, 1, 1, 0, 1, 1, 1, rel_pos), 64)


def pitch(H=256, L=1, k=9, heads=2, Hn=128, Ln=1, kn=9, nheads=2):
    return _create("pd_pitch_cond_create", _lib.pd_pitch_cond_dims(40, H, L, k, heads, Hn, Ln, kn, nheads, 1, 1), 64)


def dur(H=256, L=1, k=9, heads=2, n_layers=2, n_chans=128, kernel_size=3):
    return _create("pd_dur_create", _lib.pd_dur_dims(40, H, L, k, heads, n_layers, n_chans, kernel_size, 1.0), 64)


STACK_REJECTS = [
    (dict(H=96, heads=1), ARG, "multiple of 64"),
    (dict(H=64, heads=2), UNSUPPORTED, "head dim"),         # head dim 32
    (dict(H=192, heads=1), UNSUPPORTED, "head dim"),        # head dim 192
    (dict(k=4), ARG, "odd"),
    (dict(k=13), ARG, "<= 11"),
    (dict(L=-1), ARG, "layer count"),
]


@pytest.mark.parametrize("create", [cond, pitch, dur], ids=["pd_cond", "pd_pitch_cond", "pd_dur"])
@pytest.mark.parametrize("over,code,word", STACK_REJECTS, ids=[str(r[0]) for r in STACK_REJECTS])
def test_creates_reject_stack_dims(create, over, code, word):
    rc, msg = create(**over)
    assert rc == code and word in msg and "null parameter" not in msg, (rc, msg)


def test_creates_reject_their_own_dims():
    for over, word in ((dict(Hn=96, nheads=1), "multiple of 64"), (dict(kn=13), "<= 11"), (dict(kn=6), "odd")):
        rc, msg = pitch(**over)
        assert rc == ARG and "note encoder" in msg and word in msg, (over, rc, msg)
    for over in (dict(Hn=64, nheads=2), dict(Hn=192, nheads=1)):
        rc, msg = pitch(**over)
        assert rc == UNSUPPORTED and "note encoder" in msg and "head dim" in msg, (over, rc, msg)
    for over, word in ((dict(n_chans=48), "n_chans"), (dict(kernel_size=13), "kernel_size"),
                       (dict(kernel_size=2), "kernel_size"), (dict(n_layers=0), "n_layers")):
        rc, msg = dur(**over)
        assert rc == ARG and word in msg and "null parameter" not in msg, (over, rc, msg)
    rc, msg = cond(rel_pos=-1)
    assert rc == ARG and "rel_pos" in msg


def test_creates_accept_every_case():
    """The dims of every case, and the corners of the accepted set, get as far as the parameter list."""
    for over in (dict(H=64, heads=1, k=1, L=0), dict(H=1024, heads=4, k=11), dict(H=320, heads=5), dict(rel_pos=5003)):
        rc, msg = cond(**over)
        assert rc == ARG and "null parameter 0" in msg, (over, rc, msg)
    for n in EC.COND_CASES:
        hp = EC.hp_of("cond", n)
        rc, msg = cond(hp["hidden_size"], hp["enc_layers"], hp["enc_ffn_kernel_size"], hp["num_heads"])
        assert rc == ARG and "null parameter 0" in msg, (n, rc, msg)
    for n in EC.PITCH_CASES:
        hp = EC.hp_of("pitch", n)
        rc, msg = pitch(hp["hidden_size"], hp["enc_layers"], hp["enc_ffn_kernel_size"], hp["num_heads"],
                        hp["note_hidden_size"], hp["note_layers"], hp["note_ffn_kernel_size"], hp["note_heads"])
        assert rc == ARG and "null parameter 0" in msg, (n, rc, msg)
    for n in EC.DUR_CASES:
        hp = EC.hp_of("dur", n)
        rc, msg = dur(hp["hidden_size"], hp["enc_layers"], hp["enc_ffn_kernel_size"], hp["num_heads"], hp["n_layers"],
                      hp["n_chans"], hp["kernel_size"])
        assert rc == ARG and "null parameter 0" in msg, (n, rc, msg)
