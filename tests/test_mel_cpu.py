"""CPU checks of the mel analysis path (prodiff_amd/mel.py, pd_mel in include/prodiff_hip.h): the Slaney
filterbank pinned by its properties (the fixtures cannot pin it to librosa: tests/golden/gen_golden_mel.py
hands the reference this very function), the float64 restatement (tests/mel_ref.py) against the
reference's recorded outputs, the frame-count formula, the C-ABI's argument checks, the WAV reader and the
vocoders' wav2spec contract.  No device compute here."""
import ctypes as C
import struct

import numpy as np
import pytest
import torch

from prodiff_amd import STFT, _lib, mel_filterbank
from prodiff_amd import mel as M
from prodiff_amd import vocoder as V
from prodiff_amd.nsf_hifigan import NsfHifiGAN
from tests import mel_ref as R

fixture, restated = R.fixture, R.restated


# ---------------------------------------------------------------- filterbank
def slaney_centres(n_mels, fmin, fmax):
    """n_mels + 2 points equally spaced on Slaney's scale -- 200/3 Hz per mel below 1 kHz, ln(6.4)/27 per
    mel above -- written out independently of prodiff_amd.mel."""
    def to_mel(f):
        return f / (200 / 3) if f < 1000 else 15 + np.log(f / 1000) / (np.log(6.4) / 27)
    m = np.linspace(to_mel(fmin), to_mel(fmax), n_mels + 2)
    return np.where(m < 15, m * 200 / 3, 1000 * np.exp((m - 15) * np.log(6.4) / 27))


@pytest.mark.parametrize("sr,n_mels,fmin,fmax", [(44100, 128, 40, 16000), (22050, 80, 20, 11025), (22050, 80, 0, 8000)])
def test_filterbank_is_slaney_triangles_of_unit_area(sr, n_mels, fmin, fmax):
    """On a fine frequency grid (2^16-point FFT, so every slope holds several bins) each row is a triangle:
    two straight lines, fitted through the outermost bins of each slope, that start and end at the
    neighbouring Slaney centres, meet at the filter's own centre and enclose area 1 over Hz within 1e-6."""
    n_fft = 1 << 16
    w = M.mel_filterbank64(sr, n_fft, n_mels, fmin, fmax)
    f = np.linspace(0, sr / 2, n_fft // 2 + 1)
    pts = slaney_centres(n_mels, fmin, fmax)
    assert np.all(np.diff(pts) > 0)
    lin = pts[pts < 1000]
    np.testing.assert_allclose(np.diff(lin), np.diff(lin)[0], rtol=1e-9)          # linear below 1 kHz
    log = np.log(pts[pts >= 1000])
    np.testing.assert_allclose(np.diff(log), np.diff(log)[0], rtol=1e-9)          # logarithmic above
    for i in range(n_mels):
        row = w[i]
        nz = np.nonzero(row)[0]
        assert nz.size >= 6 and np.all(np.diff(nz) == 1), i                       # one contiguous support
        k = nz[0] + int(np.argmax(row[nz]))
        up, down = np.arange(nz[0], k), np.arange(k + 1, nz[-1] + 1)              # strictly inside each slope
        assert up.size >= 2 and down.size >= 2, i
        su = (row[up[-1]] - row[up[0]]) / (f[up[-1]] - f[up[0]])
        sd = (row[down[-1]] - row[down[0]]) / (f[down[-1]] - f[down[0]])
        assert su > 0 > sd
        np.testing.assert_allclose(row[up], row[up[0]] + su * (f[up] - f[up[0]]), rtol=0, atol=1e-12)
        np.testing.assert_allclose(row[down], row[down[0]] + sd * (f[down] - f[down[0]]), rtol=0, atol=1e-12)
        lo = f[up[0]] - row[up[0]] / su                                           # where the lines reach zero
        hi = f[down[0]] - row[down[0]] / sd
        peak_f = (sd * hi - su * lo) / (sd - su)                                  # where they meet
        height = su * (peak_f - lo)
        np.testing.assert_allclose([lo, peak_f, hi], pts[i:i + 3], rtol=1e-9, atol=1e-6)
        assert abs(0.5 * (hi - lo) * height - 1.0) <= 1e-6, i


@pytest.mark.parametrize("cfg", [R.SVS, R.TTS])
def test_filterbank_rows_at_the_working_resolution(cfg):
    """float32 of the float64 bank; rows non-negative, at most two filters per bin, every peak at the bin
    nearest to (or next to) its Slaney centre."""
    b = mel_filterbank(cfg["sr"], cfg["n_fft"], cfg["n_mels"], cfg["fmin"], cfg["fmax"])
    b64 = M.mel_filterbank64(cfg["sr"], cfg["n_fft"], cfg["n_mels"], cfg["fmin"], cfg["fmax"])
    assert b.dtype == np.float32 and b.shape == (cfg["n_mels"], cfg["n_fft"] // 2 + 1)
    np.testing.assert_array_equal(b, b64.astype(np.float32))
    assert (b >= 0).all() and ((b > 0).sum(axis=0) <= 2).all()
    df = cfg["sr"] / cfg["n_fft"]
    pts = slaney_centres(cfg["n_mels"], cfg["fmin"], cfg["fmax"])
    for i in range(cfg["n_mels"]):
        if b[i].any():
            assert abs(np.argmax(b[i]) * df - pts[i + 1]) <= df, i
    # the fixtures carry the basis the reference was handed: this one
    np.testing.assert_array_equal(fixture("base" if cfg is R.SVS else "tts")["basis"], b)


def test_stft_takes_a_basis_as_data():
    other = np.abs(np.random.default_rng(0).standard_normal((80, 513))).astype(np.float32)
    s = STFT(22050, 80, 1024, 1024, 256, 20, 11025, mel_basis=other)
    np.testing.assert_array_equal(s.mel_basis_host.numpy(), other)
    with pytest.raises(ValueError):
        STFT(22050, 80, 1024, 1024, 256, 20, 11025, mel_basis=other[:, :-1])


# ---------------------------------------------------------------- restatement and frame counts
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_float64_restatement_matches_the_reference(name):
    """tests/mel_ref.get_mel64 against the reference's own float32 outputs.  The magnitude spectrum agrees
    within 16 * 2^-24 * sum_n |y[n]| per frame -- the rounding bound of a float32 FFT of up to 4096 points
    (log2 N stages) plus the float32 window's absolute rounding (torch.hann_window cancels near its ends)
    and the products' -- and the
    log-mel within 1e-4 (the reference's error e_ref, which tests/test_gpu_mel.py scales its bar by: it
    is largest in the quiet mel bands of the harmonic signals, where the log amplifies the rounding)."""
    d = fixture(name)
    cfg, keyshift, speed, L, kinds = R.CASES[name]
    mel64, spec64, l1 = restated(name)
    assert d["mel"].shape == mel64.shape == (len(kinds), cfg["n_mels"], R.num_frames(L, cfg, keyshift, speed))
    assert d["spec"].shape == spec64.shape
    peak = np.abs(spec64).max(axis=1, keepdims=True)
    d_spec = np.abs(d["spec"] - spec64)
    e_spec = float((d_spec / np.where(peak > 0, peak, 1.0)).max())      # an all-zero frame must be exactly zero
    e_ref = float(np.abs(d["mel"] - mel64).max())
    print(f"{name}: e_spec {e_spec:.2e} of the frame peak, e_ref {e_ref:.2e}")
    assert (d_spec <= 16 * 2.0 ** -24 * l1).all()
    assert e_ref <= 1e-4
    assert np.abs(d["wav"]).max() <= 1.0


def test_frame_count_formula():
    for name, (cfg, keyshift, speed, L, kinds) in R.CASES.items():
        T = fixture(name)["mel"].shape[2]
        assert T == M.num_frames(L, cfg["n_fft"], cfg["win_size"], cfg["hop_length"], keyshift, speed), name
    assert fixture("shortest")["mel"].shape[2] == 1 and fixture("t33")["mel"].shape[2] == 33
    assert fixture("t31")["mel"].shape[2] == 31
    assert M.derived_sizes(2048, 2048, 512, 7, 1) == (3069, 3069, 512)
    assert M.derived_sizes(2048, 2048, 512, -7, 1) == (1367, 1367, 512)
    assert M.derived_sizes(2048, 2048, 512, 3, 0.8) == (2435, 2435, 410)
    s = STFT(**{k: v for k, v in R.SVS.items()})
    assert s.min_samples() == 769 and s.min_samples(12, 1) == 1793
    assert STFT(**R.SHORT_WIN).min_samples() == 424        # one whole frame: 1024 - 800 + 200


def test_zero_run_reaches_the_clip():
    d = fixture("t33")
    assert (np.abs(d["mel"][0] - np.log(1e-5)) < 2e-6).any()


# ---------------------------------------------------------------- C-ABI argument checks (no device needed)
def test_mel_exports_and_argument_checks():
    lib = _lib.lib()
    for name in ("pd_mel_create", "pd_mel_destroy", "pd_mel_frames", "pd_mel_min_samples", "pd_mel_workspace_size",
                 "pd_mel_forward"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    h = C.c_void_p(0x5a5a)
    good = _lib.pd_mel_dims(2048, 2048, 512, 128, 0.0, 1.0, 1e-5)
    assert lib.pd_mel_create(None, C.c_void_p(0x1000), None, C.byref(h)) == 1
    assert lib.pd_mel_create(C.byref(good), None, None, C.byref(h)) == 1 and b"null" in lib.pd_last_error()
    bad = [_lib.pd_mel_dims(0, 2048, 512, 128, 0.0, 1.0, 1e-5), _lib.pd_mel_dims(2048, 4096, 512, 128, 0.0, 1.0, 1e-5),
           _lib.pd_mel_dims(2048, 2048, 0, 128, 0.0, 1.0, 1e-5), _lib.pd_mel_dims(2048, 2048, 512, 0, 0.0, 1.0, 1e-5),
           _lib.pd_mel_dims(2048, 2048, 512, 128, float("nan"), 1.0, 1e-5),
           _lib.pd_mel_dims(2048, 2048, 512, 128, 0.0, 0.0, 1e-5), _lib.pd_mel_dims(2048, 2048, 512, 128, 0.0, 1.0, 0.0),
           _lib.pd_mel_dims(2048, 2048, 512, 128, 0.0, 8.0, 1e-5),      # hop 4096 > window
           _lib.pd_mel_dims(2048, 2048, 8, 128, 0.0, 1.0, 1e-5)]        # hop below 16
    for d in bad:
        assert lib.pd_mel_create(C.byref(d), C.c_void_p(0x1000), None, C.byref(h)) == 1, list(d._fields_)
    for d in (_lib.pd_mel_dims(2048, 2048, 512, 129, 0.0, 1.0, 1e-5),    # more than 128 mel bins
              _lib.pd_mel_dims(16384, 16384, 2048, 128, 0.0, 1.0, 1e-5)):   # 31 hops + a frame beyond the LDS
        assert lib.pd_mel_create(C.byref(d), C.c_void_p(0x1000), None, C.byref(h)) == 4
    assert h.value == 0x5a5a and lib.pd_live_device_bytes() == 0
    assert lib.pd_mel_forward(None, None, None, 1.0, None, None, 1, 4096, None, 0, None) == 1
    assert lib.pd_mel_frames(None, 4096) == 0 and lib.pd_mel_min_samples(None) == 0


def test_get_mel_refuses_what_it_does_not_offer():
    s = STFT(**R.SVS)
    with pytest.raises(NotImplementedError, match="center=True"):
        s.get_mel(torch.zeros(1, 4096), center=True)
    with pytest.raises(ValueError, match="at least 769"):
        s.get_mel(torch.zeros(1, 768))
    with pytest.raises(_lib.HipError, match="no CPU fallback"):
        s.get_mel(torch.zeros(1, 4096))


# ---------------------------------------------------------------- WAV reader, wav2spec
def write_wav(path, x, sr, tag, bits):
    """x [n, channels] float in [-1, 1) -> a RIFF file of PCM16 / PCM32 (tag 1) or float32 (tag 3)."""
    x = np.asarray(x, np.float64)
    if tag == 3:
        raw = x.astype("<f4").tobytes()
    else:
        raw = np.round(x * 2 ** (bits - 1)).clip(-2 ** (bits - 1), 2 ** (bits - 1) - 1).astype("<i2" if bits == 16 else "<i4").tobytes()
    ch = x.shape[1]
    fmt = struct.pack("<HHIIHH", tag, ch, sr, sr * ch * bits // 8, ch * bits // 8, bits)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"LIST" + struct.pack("<I", 3) + b"abc\0" + \
        b"data" + struct.pack("<I", len(raw)) + raw
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)


def test_read_wav_formats_and_rate_check(tmp_path):
    rng = np.random.default_rng(1)
    x = np.round(rng.uniform(-1, 1, (1000, 2)) * 32768).clip(-32768, 32767) / 32768      # exact in PCM16
    for tag, bits in ((1, 16), (1, 32), (3, 32)):
        p = str(tmp_path / f"s{tag}_{bits}.wav")
        write_wav(p, x, 44100, tag, bits)
        got = M.read_wav(p, 44100)
        assert got.dtype == np.float32 and got.shape == (1000,)
        np.testing.assert_array_equal(got, x.mean(axis=1).astype(np.float32))
    p = str(tmp_path / "mono.wav")
    write_wav(p, x[:, :1], 22050, 1, 16)
    np.testing.assert_array_equal(M.read_wav(p), x[:, 0].astype(np.float32))
    with pytest.raises(ValueError, match="sample rate 22050 differs from audio_sample_rate 44100"):
        M.read_wav(p, 44100)
    hp = dict(audio_sample_rate=44100, audio_num_mel_bins=128, fft_size=2048, win_size=2048, hop_size=512, fmin=40,
              fmax=16000)
    with pytest.raises(ValueError, match="no resampler"):
        NsfHifiGAN.wav2spec(p, hp)
    bad = str(tmp_path / "bad.wav")
    with open(bad, "wb") as f:
        f.write(b"not a wav file at all")
    with pytest.raises(ValueError, match="RIFF"):
        M.read_wav(bad)


def test_fastdiff_wav2spec_says_why():
    with pytest.raises(NotImplementedError, match="process_utterance"):
        V.FastDiff.wav2spec("x.wav", {})
