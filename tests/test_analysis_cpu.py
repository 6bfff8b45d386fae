"""CPU checks of FastDiff's analysis half (prodiff_amd/analysis.py; pd_loudness and pd_mel_create_centered_zero in
include/prodiff_hip.h): the K-weighting design and the float64 restatement tests/analysis_ref.py anchored to ITU-R
BS.1770-4 itself (its 48 kHz coefficient tables, its 997 Hz conformance reading), the block arithmetic, the gates on
the gate fixture, the refusals and the C ABI's exports and argument checks.  No device compute here."""
import ctypes as C

import numpy as np
import pytest
import prodiff_amd
from prodiff_amd import _lib
from prodiff_amd import analysis as A
from prodiff_amd import vocoder as V
from tests import analysis_ref as R

# ITU-R BS.1770-4, tables 1 and 2 (48 kHz)
BS1770_STAGE1_B = (1.53512485958697, -2.69169618940638, 1.19839281085285)
BS1770_STAGE1_A = (1.0, -1.69065929318241, 0.73248077421585)
BS1770_STAGE2_A = (1.0, -1.99004745483398, 0.99007225036621)
# What the pyloudnorm design (fc 1500 Hz / 38 Hz, Q 1/sqrt 2 / 0.5) lies away from those tables, measured here: 1.08e-4
# at the most (stage 1 b1; b0 5.8e-5, the denominators 2.4e-5 to 4.0e-5).  The bound is twice
# that: it pins the design to the recommendation's filter without claiming the two are the same numbers.
TABLE_BOUND = 2.2e-4


# ---------------------------------------------------------------- anchors outside the restatement
def test_design_matches_the_bs1770_tables_at_48k():
    k = A.kweighting_coefficients(48000)
    d = np.concatenate([k["shelf"][0] - BS1770_STAGE1_B, k["shelf"][1] - BS1770_STAGE1_A, k["pass"][1] - BS1770_STAGE2_A])
    print(f"max |design - BS.1770-4 table| at 48 kHz = {np.abs(d).max():.3e} (per coefficient {np.abs(d)})")
    assert np.abs(d).max() <= TABLE_BOUND
    # the table's stage 2 numerator is (1, -2, 1): the design's is that times (1 + cos w0) / 2 / a0, within the bound of 1
    np.testing.assert_allclose(k["pass"][0] / k["pass"][0][0], (1.0, -2.0, 1.0), rtol=0, atol=1e-15)
    assert abs(k["pass"][0][0] - 1.0) <= 5e-3
    for name, (b, a) in zip(("shelf", "pass"), R.k_filters(48000)):     # the restatement designs the same filters
        np.testing.assert_allclose(k[name][0], b, rtol=1e-14, atol=0)
        np.testing.assert_allclose(k[name][1], a, rtol=1e-14, atol=0)


@pytest.mark.parametrize("rate", [48000, 44100, 22050])
def test_full_scale_997_hz_sine_reads_minus_3_01_lkfs(rate):
    """The recommendation's conformance value for one channel, within its own +-0.1 LU."""
    x = np.sin(2 * np.pi * 997.0 * np.arange(5 * rate) / rate)
    loud = R.integrated_loudness64(x, rate)
    print(f"997 Hz full scale at {rate} Hz: {loud:.4f} LKFS")
    assert abs(loud - (-3.01)) <= 0.1


# ---------------------------------------------------------------- blocks
def test_block_bounds_are_the_expression_evaluated_in_python_floats():
    """int(0.4 * (j * 0.25) * rate), int(0.4 * (j * 0.25 + 1) * rate), hand-evaluated: the products that are not
    exact (0.4 * 0.75 * 22050 = 6615.000000000001, 0.4 * 1.75 * 44100 = 30870.000000000004) err upwards, so the
    truncation lands on rate * j / 10 and rate * (j + 4) / 10 at these rates."""
    assert A.block_bounds(22050, 6) == [(0, 8820), (2205, 11025), (4410, 13230), (6615, 15435), (8820, 17640),
                                        (11025, 19845)]
    assert A.block_bounds(44100, 4) == [(0, 17640), (4410, 22050), (8820, 26460), (13230, 30870)]
    for rate in (22050, 44100, 16000):
        T_g, step = 0.4, 0.25
        assert A.block_bounds(rate, 200) == [(int(T_g * (j * step) * rate), int(T_g * (j * step + 1) * rate))
                                             for j in range(200)]
        for L in (int(0.4 * rate) + 1, int(0.45 * rate), int(0.75 * rate), int(1.3 * rate), 7 * rate + 13):
            assert A.block_bounds(rate, A.block_count(L, rate)) == R.blocks(L, rate)
            assert A.block_count(L, rate) == int(np.round(((L / rate - T_g) / (T_g * step))) + 1)
    assert A.block_count(7200, 16000) == 1 and A.block_count(12000, 16000) == 4 and A.block_count(20800, 16000) == 10


# ---------------------------------------------------------------- fixtures
@pytest.mark.parametrize("name", sorted(R.LOUD_CASES))
def test_restatement_reproduces_the_recorded_results(name):
    d, f = R.detail(name), R.fixture(name)
    assert int(f["rate"]) == R.LOUD_CASES[name][0] and f["wav"].shape == (R.LOUD_CASES[name][1],)
    np.testing.assert_array_equal(R.case_wav(name), f["wav"])
    assert abs(d["loud"] - float(f["loud"])) <= 1e-9
    np.testing.assert_array_equal(d["abs_gate"], f["abs_gate"])
    np.testing.assert_array_equal(d["rel_gate"], f["rel_gate"])
    assert R.gate_margin(d) >= R.GATE_MARGIN
    assert R.normalize32(f["wav"], d["loud"])[1] == bool(f["peak_branch"]) == (name == "clicks")


def test_both_gates_bite_on_the_gate_fixture():
    d = R.detail("gate")
    silent, quiet, kept = ~d["abs_gate"], d["abs_gate"] & ~d["rel_gate"], d["rel_gate"]
    assert silent.sum() >= 2 and quiet.sum() >= 5 and kept.sum() >= 5
    assert (d["l"][silent] < -70.0).all() and (d["l"][quiet] <= d["gamma_r"]).all() and (d["l"][quiet] > -70.0).all()
    # each gate changes the reading: without the relative gate the quiet blocks pull it down by more than 1 dB
    ungated = -0.691 + 10 * np.log10(d["z"][d["abs_gate"]].mean())
    assert d["loud"] - ungated > 1.0
    assert ungated - (-0.691 + 10 * np.log10(d["z"].mean())) > 0.3


def test_fixture_lengths_sit_around_the_chunk_size():
    assert _lib.lib().pd_loudness_chunk() == R.CHUNK
    assert R.LOUD_CASES["chunk_x20"][1] % R.CHUNK == 0 and R.LOUD_CASES["chunk_x20m1"][1] % R.CHUNK == R.CHUNK - 1
    assert R.LOUD_CASES["r22_130"][1] % R.CHUNK not in (0, R.CHUNK - 1)


# ---------------------------------------------------------------- refusals
def test_refusals_come_before_any_device_work():
    x = np.zeros(22050, np.float32)
    with pytest.raises(NotImplementedError, match="webrtcvad"):
        A.process_utterance(x, trim_long_sil=True)
    with pytest.raises(NotImplementedError, match="webrtcvad"):
        A.process_utterance("x.wav", trim_long_sil=True)
    with pytest.raises(NotImplementedError, match="hann"):
        A.process_utterance(x, window="blackman")
    short = np.zeros(int(0.4 * 22050) - 1, np.float32)        # 8819 < 8820
    with pytest.raises(ValueError, match="greater than the block size"):
        A.process_utterance(short, loud_norm=True)
    with pytest.raises(ValueError, match="greater than the block size"):
        A.integrated_loudness(short, 22050)
    with pytest.raises(ValueError, match="greater than the block size"):
        A.normalize_loudness(np.zeros((2, 9000), np.float32), 22050, -22.0, lens=[9000, 8000])
    with pytest.raises(ValueError, match="greater than the block size"):
        R.integrated_loudness64(short, 22050)
    with pytest.raises(ValueError, match="mono"):
        A.integrated_loudness(np.zeros((2, 3, 9000), np.float32), 22050)
    assert A.min_samples(22050) == 8820 and A.min_samples(16000) == 6400


def test_fastdiff_vocoder_gains_wav2mel_and_keeps_wav2spec_refusing():
    assert callable(V.FastDiff.wav2mel) and callable(V.FastDiff.wav2wav)
    with pytest.raises(NotImplementedError, match="process_utterance"):
        V.FastDiff.wav2spec("x.wav", {})
    hp = dict(fft_size=1024, hop_size=256, win_size=1024, audio_num_mel_bins=80, fmin=80, fmax=7600,
              audio_sample_rate=22050, loud_norm=True, min_level_db=-100)
    with pytest.raises(ValueError, match="greater than the block size"):
        V.FastDiff.wav2mel(np.zeros(100, np.float32), hp)


# ---------------------------------------------------------------- exports, C-ABI argument checks (no device needed)
NEW_SYMBOLS = ("pd_mel_create_centered_zero", "pd_mel_normalize_spec", "pd_loudness_create", "pd_loudness_destroy",
               "pd_loudness_chunk", "pd_loudness_min_samples", "pd_loudness_workspace_size", "pd_loudness_forward",
               "pd_loudness_pad")


def test_exports():
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    for name in ("integrated_loudness", "normalize_loudness", "process_utterance"):
        assert name in prodiff_amd.__all__ and getattr(prodiff_amd, name) is getattr(A, name)


def test_loudness_handle_and_argument_checks():
    lib = _lib.lib()
    h = C.c_void_p(0x5a5a)
    assert lib.pd_loudness_create(None, None, C.byref(h)) == 1 and b"null" in lib.pd_last_error()
    good, _ = A._build_loudness(22050)
    for field, idx, val in (("shelf_a", 0, 2.0), ("pass_a", 2, 1.5), ("pass_b", 1, float("nan")), ("shelf_a", 1, -3.0)):
        bad, _ = A._build_loudness(22050)
        getattr(bad, field)[idx] = val
        assert lib.pd_loudness_create(C.byref(bad), None, C.byref(h)) == 1, field
    bad, _ = A._build_loudness(22050)
    bad.rate = 10
    assert lib.pd_loudness_create(C.byref(bad), None, C.byref(h)) == 1
    assert h.value == 0x5a5a
    assert lib.pd_loudness_create(C.byref(good), None, C.byref(h)) == 0      # allocates nothing on the device
    try:
        assert lib.pd_live_device_bytes() == 0
        assert lib.pd_loudness_min_samples(h) == 8820 and lib.pd_loudness_min_samples(None) == 0
        ws = lib.pd_loudness_workspace_size(h, 2, 10000, 3)
        assert ws >= 2 * 10000 * 8 and lib.pd_loudness_workspace_size(None, 2, 10000, 3) == 0
        p = C.c_void_p(0x1000)
        assert lib.pd_loudness_forward(h, None, None, p, p, 3, -22.0, p, None, None, 1, 10000, 0, p, ws, None) == 1
        assert lib.pd_loudness_forward(h, p, None, p, p, 3, -22.0, p, None, None, 1, 8819, 0, p, ws, None) == 1
        assert b"400 ms" in lib.pd_last_error()
        assert lib.pd_loudness_forward(h, p, None, p, p, 0, -22.0, p, None, None, 1, 10000, 0, p, ws, None) == 1
        assert lib.pd_loudness_forward(h, p, None, p, p, 3, float("nan"), p, None, p, 1, 10000, 10240, p, ws, None) == 1
        assert lib.pd_loudness_forward(h, p, None, p, p, 3, -22.0, p, None, None, 2, 10000, 0, p, ws - 1, None) == 3
    finally:
        lib.pd_loudness_destroy(h)
    assert lib.pd_loudness_pad(None, None, None, 1, 100, 256, None) == 1
    assert lib.pd_loudness_pad(C.c_void_p(0x1000), None, C.c_void_p(0x1000), 1, 100, 0, None) == 1


def test_centered_zero_mel_argument_checks():
    lib = _lib.lib()
    h = C.c_void_p(0x5a5a)
    good = _lib.pd_mel_dims(1024, 1024, 256, 80, 0.0, 1.0, 1e-10)
    p = C.c_void_p(0x1000)
    assert lib.pd_mel_create_centered_zero(C.byref(good), None, 1, None, C.byref(h)) == 1
    for mode in (-1, 3):
        assert lib.pd_mel_create_centered_zero(C.byref(good), p, mode, None, C.byref(h)) == 1
        assert b"out_mode" in lib.pd_last_error()
    bad = _lib.pd_mel_dims(1024, 2048, 256, 80, 0.0, 1.0, 1e-10)
    assert lib.pd_mel_create_centered_zero(C.byref(bad), p, 1, None, C.byref(h)) == 1
    assert h.value == 0x5a5a
    assert lib.pd_mel_normalize_spec(None, -100.0, None, 10, None) == 1
    assert lib.pd_mel_normalize_spec(p, 100.0, p, 10, None) == 1 and lib.pd_mel_normalize_spec(p, -100.0, p, 0, None) == 1
