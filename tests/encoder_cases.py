"""FFT-block encoder configurations away from the shipped (H, heads, k) = (256, 2, 9), one per branch of
fft_stack_forward (prodiff_amd/csrc/encoder.hip, fft_stack.h) and of the three handles built on it --
pd_cond, pd_pitch_cond, pd_dur -- that the dims and the row count select, with synthetic weights and inputs
by seed and the float64 oracle's outputs (oracle/oracle_encoder.py, tests/variance_ref.py) for them.

Nothing here needs a GPU.  The oracle outputs are computed once per process and case (lru_cache) and shared
by the fp32 and bf16 tests of tests/test_gpu_encoder_dims.py; callers must not modify the arrays.

Every batch is padded (pad_tokens >= 1 zero tokens after the longest row) and ragged.  A condition case
with ``txt_lens`` hands each row's phoneme count to the kernels: the oracle then runs each row alone, which
is what the padded batch has to equal on that row's own tokens and frames (include/prodiff_hip.h).  Without
it the oracle runs the padded batch as the reference does.

enc_big_tile / enc_ksplit restate fft_stack.h:95-102, so each case states which tile every one of its GEMMs
takes (``big``: the names of the GEMMs on the 128 x 64 tile; all others run 32 x 128 split-K tiles) and
tests/test_encoder_dims_cpu.py keeps a later change of lengths from dropping a case off its branch.

The small cases also have fixtures, tests/golden/encdims_<family>_<name>.npz, with the reference modules' own outputs
(tests/golden/gen_golden.py:gen_encdims, gen_golden_variance.py); the row-count cases and the 5,003-token
call run the default dims and have none.
"""
from functools import lru_cache

import numpy as np

from oracle import oracle_encoder as OE
from prodiff_amd import synth
from tests import golden_io as G
from tests import variance_cases as VC
from tests import variance_ref as VR

VOCAB = VC.VOCAB
DUR_BIAS = VC.DUR_BIAS
GEMM_BK = 32        # gemm.h
AK = 32             # keys per chunk of enc_attn_kernel (encoder.hip)

_OFF = dict(use_spk_id=False, use_lang_id=False, use_voicing_embed=False, use_breath_embed=False)
_L8096 = [252] * 8 + [60 + 8 * i for i in range(24)]     # + 1 padding token: 32 x 253 = 8096 rows

# name: hp over synth.COND_DEFAULTS with enc_layers 1, the rows' phoneme counts, padding, and the branch
COND_CASES = {
    # head dim 64 over two key chunks (the online-softmax carry); one row is shorter than a chunk
    "h64_d64": dict(hp=dict(hidden_size=64, num_heads=1, enc_ffn_kernel_size=3), lengths=[44, 20], pad_tokens=1),
    # three key chunks
    "h128_d64": dict(hp=dict(hidden_size=128, num_heads=2), lengths=[69, 33], pad_tokens=1),
    # N = 576 and 768 are no multiples of the 128-wide tile: the column masking
    "h192_d64": dict(hp=dict(hidden_size=192, num_heads=3, enc_ffn_kernel_size=5, enc_layers=2), lengths=[37, 12],
                     pad_tokens=2),
    "h320_d64": dict(hp=dict(hidden_size=320, num_heads=5, enc_ffn_kernel_size=7), lengths=[37, 12], pad_tokens=1),
    "h512_d256": dict(hp=dict(hidden_size=512, num_heads=2, enc_ffn_kernel_size=1), lengths=[33, 9], pad_tokens=1),
    "h512_d128": dict(hp=dict(hidden_size=512, num_heads=4, enc_ffn_kernel_size=11, enc_layers=4), lengths=[33, 9],
                      pad_tokens=3),
    # the five right-hand taps cross every row's own end
    "k11": dict(hp=dict(enc_ffn_kernel_size=11), lengths=[37, 12, 29], pad_tokens=6, txt_lens=True),
    "k1": dict(hp=dict(enc_ffn_kernel_size=1), lengths=[37, 12], pad_tokens=1),
    # embedding, then the final LayerNorm only
    "l0": dict(hp=dict(enc_layers=0), lengths=[17, 9], pad_tokens=2),
    # one token per row, 1..3 frames
    "t1": dict(hp=dict(), lengths=[1, 1, 1], pad_tokens=0, frames=[1, 2, 3]),
    # the create walk without the optional tables; enc_cond_kernel without speaker and variance terms
    "flags_min": dict(hp=dict(_OFF), lengths=[17, 9], pad_tokens=2),
    # enc_cond_kernel's breath-only branch
    "breath_only": dict(hp=dict(use_voicing_embed=False), lengths=[17, 9], pad_tokens=2),
    # 2000 rows: the FFN conv (N = 1024) takes the 128 x 64 tile with ragged lens, the other three stay split-K
    "rows2000": dict(hp=dict(enc_ffn_kernel_size=3), lengths=[249, 248, 180, 249, 33, 249, 101, 249], pad_tokens=1,
                     txt_lens=True, max_dur=2, big=("ffn1",), fixture=False),
    # 8096 rows: all four GEMMs take the 128 x 64 tile
    "rows8096": dict(hp=dict(enc_ffn_kernel_size=1), lengths=_L8096, pad_tokens=1, max_dur=2,
                     big=("qkv", "outproj", "ffn1", "ffn2"), fixture=False),
}
# RelPositionalEncoding whose table a real batch grew: a B = 1 batch of RELPOS_LONG tokens goes through the
# module, then the short batch, which counts its reversed positions from RELPOS_LONG
RELPOS_LONG = 5003
RELPOS_HP = dict(hidden_size=64, num_heads=1, enc_ffn_kernel_size=1, rel_pos=True, num_spk=2)
RELPOS_CASES = {
    "relpos_over_table": dict(hp=RELPOS_HP, lengths=[RELPOS_LONG], pad_tokens=0, max_dur=1, fixture=False),
    "relpos_after": dict(hp=dict(RELPOS_HP, rel_pos_len=RELPOS_LONG), lengths=[21, 13], pad_tokens=1, fixture=False,
                         params_of="relpos_over_table"),
}

_PSMALL = dict(lengths=[17, 9, 23], note_lengths=[7, 4, 10], pad_tokens=2, pad_notes=1)
# name: hp over synth.PITCH_DEFAULTS with enc_layers 1 and note_layers 1
PITCH_CASES = {
    # note_encode_out_linear with K = 64: two K steps, no split
    "note64": dict(hp=dict(hidden_size=128, num_heads=2, note_hidden_size=64, note_heads=1, note_ffn_kernel_size=3,
                           num_spk=3), **_PSMALL),
    "note256_d64": dict(hp=dict(hidden_size=192, num_heads=3, note_hidden_size=256, note_heads=4, num_spk=3),
                        **_PSMALL),
    "note_l0": dict(hp=dict(note_layers=0, num_spk=3), **_PSMALL),
    "tn1": dict(hp=dict(num_spk=2), lengths=[1, 1], note_lengths=[1, 1], pad_tokens=0, pad_notes=0),
    "nospk": dict(hp=dict(hidden_size=64, num_heads=1, use_spk_id=False), **_PSMALL),
}

# name: hp over synth.DUR_DEFAULTS with enc_layers 1
DUR_CASES = {
    "c32_k11": dict(hp=dict(hidden_size=64, num_heads=1, n_chans=32, kernel_size=11, n_layers=1),
                    lengths=[17, 9, 23], pad_tokens=2),
    "c96_k5": dict(hp=dict(n_chans=96, kernel_size=5, n_layers=3), lengths=[17, 9, 23], pad_tokens=2),
    "c512_k1": dict(hp=dict(n_chans=512, kernel_size=1, n_layers=2), lengths=[17, 9, 23], pad_tokens=2),
    # 8096 rows: dur_conv takes the 128 x 64 tile (no encoder layers: the convs read the embedding's LayerNorm)
    "dur_rows8096": dict(hp=dict(enc_layers=0, n_layers=2, n_chans=512, kernel_size=3), lengths=_L8096,
                         pad_tokens=1, big=("dur_conv0", "dur_conv"), fixture=False),
}

FAMILIES = {"cond": dict(COND_CASES, **RELPOS_CASES), "pitch": PITCH_CASES, "dur": DUR_CASES}
_DEFAULTS = {"cond": dict(synth.COND_DEFAULTS, enc_layers=1, num_spk=3, num_langs=3),
             "pitch": dict(synth.PITCH_DEFAULTS, enc_layers=1, note_layers=1),
             "dur": dict(synth.DUR_DEFAULTS, enc_layers=1)}


def case(family, name):
    return FAMILIES[family][name]


def fixture_cases(family):
    """The cases with a fixture of the reference's outputs."""
    return [n for n, c in FAMILIES[family].items() if c.get("fixture", True)]


def hp_of(family, name):
    return dict(_DEFAULTS[family], **case(family, name)["hp"])


def seed_of(family, name):
    return 5000 + 1000 * list(FAMILIES).index(family) + 10 * list(FAMILIES[family]).index(name)


# ---------------------------------------------------------------- the tile every GEMM takes (fft_stack.h:95-102)
def cdiv(a, b):
    return -(-a // b)


def enc_big_tile(rows, N):
    """fft_stack.h:95: 128 x 64 tiles once they give every CU a block."""
    return cdiv(rows, 128) * cdiv(N, 64) >= 256


def enc_ksplit(rows, N, K):
    """fft_stack.h:96-102: the K axis of the 32 x 128 tiles split over up to 8 blocks, >= 4 K steps each."""
    if enc_big_tile(rows, N):
        return 1
    gxy = cdiv(rows, 32) * cdiv(N, 128)
    ks = min(8, (256 + gxy - 1) // gxy)
    ks = min(ks, max(1, K // GEMM_BK // 4))
    return max(ks, 1)


def stack_gemms(H, k, prefix=""):
    """{name: (N, K)} of one FFT block's four GEMMs (fft_stack_forward)."""
    return {prefix + "qkv": (3 * H, H), prefix + "outproj": (H, H), prefix + "ffn1": (4 * H, k * H),
            prefix + "ffn2": (H, 4 * H)}


def gemms(family, name):
    """{GEMM: (rows, N, K)} of a case's forward: the stacks' (none of a stack without layers), then the
    handle's own."""
    c, hp = case(family, name), hp_of(family, name)
    B = len(c["lengths"])
    rows = B * (max(c["lengths"]) + c["pad_tokens"])
    out = {}
    if hp["enc_layers"]:
        out.update({g: (rows,) + nk for g, nk in stack_gemms(hp["hidden_size"], hp["enc_ffn_kernel_size"]).items()})
    if family == "pitch":
        nrows = B * (max(c["note_lengths"]) + c["pad_notes"])
        if hp["note_layers"]:
            out.update({g: (nrows,) + nk for g, nk in
                        stack_gemms(hp["note_hidden_size"], hp["note_ffn_kernel_size"], "note_").items()})
        out["note_out"] = (nrows, hp["hidden_size"], hp["note_hidden_size"])
    if family == "dur":
        out["dur_conv0"] = (rows, hp["n_chans"], hp["kernel_size"] * hp["hidden_size"])
        if hp["n_layers"] > 1:
            out["dur_conv"] = (rows, hp["n_chans"], hp["kernel_size"] * hp["n_chans"])
    return out


def tiles(family, name):
    """{GEMM: 'big' | ksplit} as enc_gemm chooses."""
    return {g: "big" if enc_big_tile(r, N) else enc_ksplit(r, N, K) for g, (r, N, K) in gemms(family, name).items()}


def key_chunks(family, name):
    c = case(family, name)
    return cdiv(max(c["lengths"]) + c["pad_tokens"], AK)


# ---------------------------------------------------------------- the workspace the handles ask for
def _al(n):
    return (n + 63) // 64 * 64


def _part(rows, N, K):
    """enc_part_floats (fft_stack.h:104-107): floats of split-K partial sums, none on the 128 x 64 tile."""
    ks = enc_ksplit(rows, N, K)
    return ks * rows * N if ks > 1 else 0


def _fft_ws(R, H, k):
    """fft_ws (encoder.hip): mask, x, h, qkv, att, f and the largest partial-sum buffer of the four GEMMs."""
    part = max(_part(R, N, K) for N, K in stack_gemms(H, k).values())
    return _al(R) + 3 * _al(R * H) + _al(3 * R * H) + _al(4 * R * H) + _al(part)


def workspace_bytes(family, name):
    """pd_cond / pd_pitch_cond / pd_dur _workspace_size for the case's batch, restated from cond_ws (encoder.hip),
    pitch_ws and dur_ws (variance.hip).  It depends on enc_ksplit through the partial-sum buffers, so the
    library returning this number ties the restated tile choice above to the one the kernels are launched with."""
    c, hp = case(family, name), hp_of(family, name)
    B, H, k = len(c["lengths"]), hp["hidden_size"], hp["enc_ffn_kernel_size"]
    R = B * (max(c["lengths"]) + c["pad_tokens"])
    n = _fft_ws(R, H, k) + _al(R * H)
    if family == "pitch":
        Rn, Hn = B * (max(c["note_lengths"]) + c["pad_notes"]), hp["note_hidden_size"]
        n += _fft_ws(Rn, Hn, hp["note_ffn_kernel_size"]) + _al(Rn * Hn) + _al(Rn * H) + _al(_part(Rn, H, Hn))
    if family == "dur":
        C, kd = hp["n_chans"], hp["kernel_size"]
        n += 2 * _al(R * C) + _al(max(_part(R, C, kd * H), _part(R, C, kd * C)))
    return 4 * n


# ---------------------------------------------------------------- weights and inputs
@lru_cache(maxsize=None)
def params(family, name):
    """The reference state dict of a case (of the case ``params_of`` names: the same module, another batch)."""
    name = case(family, name).get("params_of", name)
    hp, s = hp_of(family, name), seed_of(family, name)
    if family == "cond":
        return synth.synth_cond_params(synth.cond_param_shapes(VOCAB, **hp), s)
    if family == "pitch":
        return synth.synth_variance_params(synth.pitch_param_shapes(VOCAB, **hp), s)
    return synth.synth_variance_params(synth.dur_param_shapes(VOCAB, **hp), s, DUR_BIAS)


@lru_cache(maxsize=None)
def inputs(family, name):
    """The forward's keyword arguments as numpy arrays (only those the case's flags take)."""
    c, hp, s = case(family, name), hp_of(family, name), seed_of(family, name) + 1
    if family == "pitch":
        x = synth.synth_pitch_inputs(s, c["lengths"], c["note_lengths"], VOCAB, hp["num_spk"], c["pad_tokens"],
                                     c["pad_notes"])
        if not hp["use_spk_id"]:
            x.pop("spk_id")
        return x
    if family == "dur":
        return synth.synth_dur_inputs(s, c["lengths"], VOCAB, c["pad_tokens"])
    x = synth.synth_cond_inputs(s, c["lengths"], VOCAB, hp["num_spk"], hp["num_langs"], c.get("max_dur", 3),
                                c["pad_tokens"])
    if "frames" in c:   # one token per row: row b lasts frames[b] frames
        Tm = max(c["frames"])
        wide = synth.synth_cond_inputs(s, [Tm] * len(c["lengths"]), VOCAB, max_dur=1)   # curves of Tm frames
        x["mel2ph"] = (np.arange(Tm)[None, :] < np.array(c["frames"])[:, None]).astype(np.int64)
        x.update({k: wide[k] for k in ("f0", "voicing", "breath")})
    for key, flag in (("lang_seq", "use_lang_id"), ("spk_embed_id", "use_spk_id"), ("voicing", "use_voicing_embed"),
                      ("breath", "use_breath_embed")):
        if not hp[flag]:
            x.pop(key)
    return x


def cond_row_alone(ins, b, n_tok):
    """Row b of a padded condition batch as the segment alone: its own tokens and frames only."""
    frames = int((ins["mel2ph"][b] > 0).sum())
    out = {}
    for k, v in ins.items():
        r = v[b:b + 1]
        if k in ("txt_tokens", "lang_seq"):
            r = r[:, :n_tok]
        elif k in ("mel2ph", "f0", "voicing", "breath"):
            r = r[:, :frames]
        out[k] = np.ascontiguousarray(r)
    return out


def lens_of(family, name):
    """(txt_lens, note_lens or None) of a case's rows."""
    c = case(family, name)
    return list(c["lengths"]), (list(c["note_lengths"]) if "note_lengths" in c else None)


# ---------------------------------------------------------------- float64 oracle outputs
@lru_cache(maxsize=None)
def cond_ref(name):
    """(cond, enc) of the padded batch; with txt_lens, per row (cond [frames_b, H], enc [lengths[b], H]) of the
    row alone."""
    c, hp, P, x = case("cond", name), hp_of("cond", name), params("cond", name), inputs("cond", name)
    if not c.get("txt_lens"):
        return OE.forward_condition(P, hp, return_encoder=True, **x)
    rows = [OE.forward_condition(P, hp, return_encoder=True, **cond_row_alone(x, b, n))
            for b, n in enumerate(c["lengths"])]
    return [r[0][0] for r in rows], [r[1][0] for r in rows]


def cond_valid(name, cond, enc):
    """A padded batch's (cond, enc) cut to what cond_ref returns; the rest of a txt_lens batch must be zero."""
    c = case("cond", name)
    if not c.get("txt_lens"):
        return cond, enc
    frames = (inputs("cond", name)["mel2ph"] > 0).sum(1)
    return ([cond[b, :f] for b, f in enumerate(frames)], [enc[b, :n] for b, n in enumerate(c["lengths"])])


@lru_cache(maxsize=None)
def pitch_ref(name):
    return VR.pitch_condition(params("pitch", name), hp_of("pitch", name), **inputs("pitch", name))


@lru_cache(maxsize=None)
def dur_ref(name):
    """(durations, log-domain output) [B, T_txt]."""
    return VR.dur_forward(params("dur", name), hp_of("dur", name), **inputs("dur", name))


# ---------------------------------------------------------------- the reference's hparams and its fixtures
def teacher_hparams(hp):
    """The reference ProDiffTeacher's hparams for a case's hp (a one-layer denoiser: only the condition runs)."""
    return dict({k: v for k, v in hp.items() if k != "rel_pos_len"}, audio_num_mel_bins=128, dropout=0.1,
                languages=["l%d" % i for i in range(hp["num_langs"] - 1)], residual_layers=1, residual_channels=64,
                dilation_cycle_length=1, timesteps=4, timescale=1000, schedule_type="vpsde", max_beta=40.0,
                spec_min=[-12], spec_max=[0])


def fixture(family, name):
    """tests/golden/encdims_<family>_<name>.npz: the inputs and the reference module's outputs."""
    return G.load(f"encdims_{family}_{name}")
