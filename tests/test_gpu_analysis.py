"""GPU tests of FastDiff's analysis half (prodiff_amd.analysis on pd_loudness and pd_mel_create_centered_zero;
FastDiff.wav2mel / wav2wav) against the float64 restatement tests/analysis_ref.py and the fixtures
tests/golden/analysis_*.npz.

Bars:
 (i)   loudness: |native - float64| <= LOUD_BAR dB.  Measured over the ten fixtures on an MI355X: 1.6e-14 dB at the
       most (nine ulp of a reading near -13; six of the ten agree to the last bit).  The bar is
       ten times that.  It may never be looser than 1e-4 dB, which would move every mel value by 1.15e-5 relative, a
       tenth of the project's 1e-4 bar.
 (ii)  magnitude spectrum: |d| <= 1e-5 * the frame's peak (tests/test_gpu_mel.py's bar);
 (iii) linear mel: |d| <= 1e-4 * the frame's peak mel; log10 mel: |d| <= 1e-4 where the mel exceeds 10 eps;
 (iv)  the returned waveform equals the restatement's exactly with loud_norm off; with it on the two gains are the
       float32 roundings of two doubles a few 1e-13 apart, so the samples agree within one float32 rounding of the
       gain and one of the product (2.4e-7 relative) -- and exactly with the gain taken from the native loudness;
 (v)   the normalised return_linear spectrum against its formula applied in float64 to the native magnitude:
       20 log10f of a value of at most 100 is good to 2 ulp (1.5e-5), the division by 100 leaves 1.5e-7, two more
       float32 roundings of a result of at most 2 add 2.4e-7: 5e-7.
"""
import functools

import numpy as np
import pytest
import torch

from prodiff_amd import analysis as A
from tests import analysis_ref as R

pytestmark = pytest.mark.gpu

LOUD_BAR = 1.6e-13
assert LOUD_BAR <= 1e-4
F32_TWO_ROUNDINGS = 2.4e-7


def cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


# ---------------------------------------------------------------- a. loudness
@pytest.mark.parametrize("name", sorted(R.LOUD_CASES))
def test_loudness_matches_the_restatement(name):
    rate = R.LOUD_CASES[name][0]
    wav, d = R.fixture(name)["wav"], R.detail(name)
    loud = A.integrated_loudness(wav, rate)
    assert isinstance(loud, float)
    on_device = A.integrated_loudness(cuda(wav), rate)
    assert on_device.dtype == torch.float64 and on_device.is_cuda and float(on_device) == loud
    print(f"{name}: native {loud:.12f} float64 {d['loud']:.12f} |d| = {abs(loud - d['loud']):.3e} dB "
          f"({len(d['z'])} blocks, {int(d['rel_gate'].sum())} kept)")
    assert abs(loud - d["loud"]) <= LOUD_BAR


def test_silence_reads_minus_infinity():
    assert A.integrated_loudness(np.zeros(9000, np.float32), 22050) == -np.inf


# ---------------------------------------------------------------- b. gain and peak branch
@pytest.mark.parametrize("name", ["clicks", "r22_130", "gate"])
def test_gain_and_peak_branch(name):
    rate = R.LOUD_CASES[name][0]
    wav, d = R.fixture(name)["wav"], R.detail(name)
    out = A.normalize_loudness(wav, rate, -22.0)
    assert out.dtype == np.float32 and out.shape == wav.shape
    ref, took = R.normalize32(wav, d["loud"], -22.0)
    assert took == (name == "clicks")
    if took:
        assert np.abs(out).max() == 1.0                       # divided by its own peak
    else:
        assert np.abs(out).max() < 1.0
    np.testing.assert_allclose(out, ref, rtol=F32_TWO_ROUNDINGS, atol=0)
    # the float32 arithmetic itself, from the native loudness: exact
    np.testing.assert_array_equal(out, R.normalize32(wav, A.integrated_loudness(wav, rate), -22.0)[0])


# ---------------------------------------------------------------- c. mel and spectrum
@functools.lru_cache(maxsize=None)
def native(name, loud_norm, vocoder):
    eps = 1e-6 if vocoder == "pwg" else 1e-10
    wav, mel, spc = A.process_utterance(R.fixture(name)["wav"], loud_norm=loud_norm, vocoder=vocoder, eps=eps,
                                        return_linear=True, **R.TTS)
    # the raw magnitude of the same waveform, from the same front end
    hp = R.TTS
    front = A._front(hp["sample_rate"], hp["fft_size"], hp["hop_size"], hp["win_length"], hp["num_mels"],
                     float(hp["fmin"]), float(hp["fmax"]), float(eps), vocoder == "pwg")
    L = R.LOUD_CASES[name][1]
    _, mag = front._mel_time_major(cuda(wav)[None], 0, 1, lens=[L], return_spec=True)
    return wav, mel, spc, mag[0, :mel.shape[1]].cpu().numpy().T


@pytest.mark.parametrize("vocoder", ["fastdiff", "pwg"])
@pytest.mark.parametrize("loud_norm", [False, True])
@pytest.mark.parametrize("name", R.MEL_CASES)
def test_process_utterance(name, loud_norm, vocoder):
    L, hop = R.LOUD_CASES[name][1], R.TTS["hop_size"]
    T = 1 + L // hop
    ref = R.restated(name, loud_norm, vocoder)
    lin = R.restated(name, loud_norm, "fastdiff")["mel"]
    wav, mel, spc, mag = native(name, loud_norm, vocoder)
    assert wav.shape == (T * hop,) and mel.shape == (80, T) and spc.shape == (513, T) and mag.shape == (513, T)
    assert wav.dtype == mel.dtype == spc.dtype == np.float32
    assert np.isfinite(mel).all() and np.isfinite(spc).all()
    if loud_norm:
        np.testing.assert_allclose(wav, ref["wav"], rtol=F32_TWO_ROUNDINGS, atol=0)
        assert ref["peak_branch"] == (name == "clicks") and (np.abs(wav).max() == 1.0) == ref["peak_branch"]
    else:
        np.testing.assert_array_equal(wav, ref["wav"])
    assert (wav[L:] == 0).all()
    peak = ref["mag"].max(axis=0, keepdims=True)
    d_mag = np.abs(mag - ref["mag"])
    print(f"{name} loud_norm={loud_norm} {vocoder}: spectrum max|d| / frame peak = "
          f"{float((d_mag / np.where(peak > 0, peak, 1.0)).max()):.2e}", end="")
    assert (d_mag <= 1e-5 * peak).all()
    if vocoder == "fastdiff":
        mpeak = ref["mel"].max(axis=0, keepdims=True)
        d_mel = np.abs(mel - ref["mel"])
        print(f", mel max|d| / frame peak mel = {float((d_mel / np.where(mpeak > 0, mpeak, 1.0)).max()):.2e}", end="")
        assert (d_mel <= 1e-4 * mpeak).all()
    else:
        eps = 1e-6
        above = lin > 10 * eps
        d_log = np.abs(mel - ref["mel"])
        print(f", log10 mel max|d| above 10 eps = {float(d_log[above].max()):.2e} ({int(above.sum())} of {above.size})",
              end="")
        assert above.any() and (d_log[above] <= 1e-4).all()
        assert (mel >= np.float32(np.log10(eps)) - 1e-6).all()
    spc64 = (20 * np.log10(np.maximum(1e-5, mag.astype(np.float64))) + 100.0) / 100.0
    print(f", normalised spectrum max|d| = {float(np.abs(spc - spc64).max()):.2e}")
    assert np.abs(spc - spc64).max() <= 5e-7


def test_device_tensors_in_and_out():
    x = cuda(R.fixture("r22_045")["wav"])
    wav, mel = A.process_utterance(x, vocoder="fastdiff", eps=1e-10, to_numpy=False, **R.TTS)
    ref = native("r22_045", False, "fastdiff")
    assert wav.is_cuda and mel.is_cuda and mel.shape == (80, 39)
    np.testing.assert_array_equal(wav.cpu().numpy(), ref[0])
    np.testing.assert_array_equal(mel.cpu().numpy(), ref[1])


# ---------------------------------------------------------------- d. ragged batch
RAGGED = ("r22_045", "r22_130", "chunk_x20m1")       # 9922, 28665 and 10239 samples at 22.05 kHz


def test_ragged_rows_equal_the_rows_alone():
    clips = [R.fixture(n)["wav"] for n in RAGGED]
    lens = [len(c) for c in clips]
    alone_loud = [A.integrated_loudness(cuda(c), 22050) for c in clips]
    alone_norm = [A.normalize_loudness(cuda(c), 22050, -22.0) for c in clips]
    alone = [A.process_utterance(cuda(c), loud_norm=True, vocoder="fastdiff", eps=1e-10, return_linear=True,
                                 to_numpy=False, **R.TTS) for c in clips]
    for order in ([0, 1, 2], [2, 0, 1], [1, 2, 0]):
        L = max(lens)
        batch = np.full((3, L), np.nan, np.float32)           # what lies past a row's length must not be read
        for row, i in enumerate(order):
            batch[row, :lens[i]] = clips[i]
        ln = [lens[i] for i in order]
        loud = A.integrated_loudness(cuda(batch), 22050, lens=ln)
        norm = A.normalize_loudness(cuda(batch), 22050, -22.0, lens=ln)
        wavs, mels, spcs = A.process_utterance(cuda(batch), lens=ln, loud_norm=True, vocoder="fastdiff", eps=1e-10,
                                               return_linear=True, to_numpy=False, **R.TTS)
        listed = A.process_utterance([cuda(clips[i]) for i in order], loud_norm=True, vocoder="fastdiff", eps=1e-10,
                                     return_linear=True, to_numpy=False, **R.TTS)
        for row, i in enumerate(order):
            assert torch.equal(loud[row], alone_loud[i]), (order, i)
            assert torch.equal(norm[row, :lens[i]], alone_norm[i]) and (norm[row, lens[i]:] == 0).all(), (order, i)
            for got, lst, want in zip((wavs[row], mels[row], spcs[row]), (listed[0][row], listed[1][row], listed[2][row]),
                                      alone[i]):
                assert got.shape == want.shape and torch.equal(got, want), (order, i)
                assert torch.equal(lst, want), (order, i)


# ---------------------------------------------------------------- e. copy synthesis
def test_wav2mel_and_wav2wav_on_a_synthetic_model():
    from prodiff_amd import FastDiff, synth
    from prodiff_amd import vocoder as V
    hp = dict(fft_size=1024, hop_size=256, win_size=1024, audio_num_mel_bins=80, fmin=80, fmax=7600,
              audio_sample_rate=22050, loud_norm=True, min_level_db=-100)
    x = R.fixture("r22_045")["wav"]
    T = 1 + len(x) // 256
    wav, mel, spc = V.FastDiff.wav2mel(x, hp, return_linear=True)
    ref = native("r22_045", True, "fastdiff")
    assert mel.shape == (T, 80) and spc.shape == (T, 513)
    np.testing.assert_array_equal(wav, ref[0])
    np.testing.assert_array_equal(mel, ref[1].T)
    np.testing.assert_array_equal(spc, ref[2].T)
    fd = FastDiff()
    fd.load_state_dict({k: torch.from_numpy(v) for k, v in
                        synth.synth_params(synth.fastdiff_param_shapes(), 31).items()})
    voc = V.FastDiff(hp, model=fd.cuda())
    out = voc.wav2wav(x, seed=3)
    assert out.shape == (T * 256,) and out.dtype == np.float32 and np.isfinite(out).all()
