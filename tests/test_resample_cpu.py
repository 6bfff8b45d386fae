"""CPU checks of the sample-rate conversion (prodiff_amd/resample.py, pd_resample in include/prodiff_hip.h): the
host-side float64 table against the independent restatement (tests/resample_ref.py), the definition against
scipy.signal.upfirdn, the output length, a sine through the float64 definition, the C-ABI's argument checks and
the Python layer's contract.  No device compute here."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from prodiff_amd import KAISER_BEST, Resample, _lib, sinc_resample_kernel64
from prodiff_amd import mel as M
from prodiff_amd import resample as RS
from prodiff_amd.nsf_hifigan import NsfHifiGAN
from tests import resample_ref as R
from tests.test_mel_cpu import write_wav

CASE_NAMES = sorted(R.CASES)


def test_kaiser_best_parameters():
    assert KAISER_BEST == R.KAISER_BEST and RS.DEFAULT_BETA == R.BETA


@pytest.mark.parametrize("name", CASE_NAMES)
def test_table_matches_the_restatement(name):
    orig, new, kw, dims = R.CASES[name]
    h, W, o, n = sinc_resample_kernel64(orig, new, **kw)
    ref, Wr, o_r, n_r = R.table64(orig, new, **kw)
    assert (W, o, n) == (Wr, o_r, n_r) and h.dtype == np.float64 and h.shape == ref.shape == (n, 2 * W + o)
    if dims is not None:
        assert (o, n, W, 2 * W + o) == dims
    assert np.abs(h - ref).max() <= 1e-15
    base = min(o, n) * kw.get("rolloff", 0.99)
    assert h[0][W] == base / o                       # t = 0: sinc 1, window 1
    r = Resample(orig, new, **kw)
    assert (r.o, r.n, r.width) == (o, n, W)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_direct_sum_equals_upfirdn(name):
    orig, new, kw, _ = R.CASES[name]
    h, W, o, n = R.table64(orig, new, **kw)
    rng = np.random.default_rng(ord(name))
    for L in (1, o + 1, 5 * o + 3):
        x = rng.uniform(-1, 1, L)
        a = R.direct64(x, h, W, o, n)[0]
        b = R.upfirdn64(x, h, W, o, n)
        assert a.shape == b.shape and np.abs(a - b).max() <= 1e-12, (L, np.abs(a - b).max())


@pytest.mark.parametrize("name", CASE_NAMES)
def test_output_length(name):
    orig, new, kw, _ = R.CASES[name]
    h, W, o, n = R.table64(orig, new, **kw)
    r = Resample(orig, new, **kw)
    for L in sorted({1, max(o - 1, 1), o, o + 1, 33 * o + 5}):
        want = -(-n * L // o)
        assert want == math.ceil(n * L / o)
        assert R.direct64(np.zeros(L), h, W, o, n).shape == (1, want)
        assert r.out_samples(L) == want
    assert r.out_samples(2 ** 31 - 1) == -(-n * (2 ** 31 - 1) // o)      # beyond 32 bits when upsampling


# float64 distance of the definition from the analytic sine in the middle half of the output, as measured when the
# definition was written down (2-3e-4 at width 6 with the Hann window, 5e-8 at widths 16, 64 and 128), times 2.
# Case d (Kaiser window at width 6) has no such figure and is left out: a bar for it would have to come from this
# very computation.
SINE_BAR = {"a": 6e-4, "b": 1e-7, "c": 6e-4, "e": 1e-7, "f": 1e-7}


@pytest.mark.parametrize("name", sorted(SINE_BAR))
def test_sine_in_sine_out(name):
    """A sine at 5 % of the lower rate comes out as the same sine at the new rate."""
    orig, new, kw, _ = R.CASES[name]
    h, W, o, n = R.table64(orig, new, **kw)
    f = 0.05 * min(orig, new)
    L = 40 * o + 8 * W
    x = np.sin(2 * np.pi * f * np.arange(L) / orig)
    y = R.direct64(x, h, W, o, n)[0]
    want = np.sin(2 * np.pi * f * np.arange(len(y)) / new)
    mid = slice(len(y) // 4, 3 * len(y) // 4)
    err = float(np.abs(y[mid] - want[mid]).max())
    print(f"{name}: {err:.2e}")
    assert err <= SINE_BAR[name]


# ---------------------------------------------------------------- C-ABI argument checks (no device needed)
def dims(orig=48000, new=44100, width=6, rolloff=0.99, method=0, beta=R.BETA):
    return _lib.pd_resample_dims(orig, new, width, rolloff, method, beta)


def test_resample_exports_and_argument_checks():
    lib = _lib.lib()
    for name in ("pd_resample_create", "pd_resample_destroy", "pd_resample_out_samples", "pd_resample_taps",
                 "pd_resample_kernel", "pd_resample_workspace_size", "pd_resample_forward"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    h = C.c_void_p(0x5a5a)
    good = dims()
    assert lib.pd_resample_create(None, None, C.byref(h)) == 1 and b"null" in lib.pd_last_error()
    assert lib.pd_resample_create(C.byref(good), None, None) == 1
    bad = [dims(orig=0), dims(new=0), dims(orig=-48000), dims(new=-1), dims(width=0), dims(width=-6),
           dims(rolloff=0.0), dims(rolloff=-0.5), dims(rolloff=float("nan")), dims(method=2), dims(method=-1),
           dims(method=1, beta=-1.0), dims(method=1, beta=float("nan"))]
    for d in bad:
        assert lib.pd_resample_create(C.byref(d), None, C.byref(h)) == 1, [getattr(d, f[0]) for f in d._fields_]
    for d in (dims(44100, 44101),                     # o = 44100: 32 frames of it are far beyond the LDS
              dims(1, 44101),                         # n = 44101: so is the output tile
              dims(48000, 44100, width=20000)):       # the halo alone is
        assert lib.pd_resample_create(C.byref(d), None, C.byref(h)) == 4 and b"fit" in lib.pd_last_error()
    assert h.value == 0x5a5a and lib.pd_live_device_bytes() == 0
    assert lib.pd_resample_forward(None, None, None, None, 1, 4096, None, 0, None) == 1
    assert lib.pd_resample_out_samples(None, 4096) == 0
    assert lib.pd_resample_workspace_size(None, 1, 4096) == 0
    assert lib.pd_resample_taps(None, None, None, None) == 1
    assert lib.pd_resample_kernel(None, None, None) == 1


# ---------------------------------------------------------------- Python layer
def test_resample_refuses_a_cpu_tensor_and_returns_equal_rates_unchanged():
    with pytest.raises(_lib.HipError, match="no CPU fallback"):
        Resample(48000, 44100)(torch.zeros(1, 4096))
    with pytest.raises(_lib.HipError, match="no CPU fallback"):
        RS.resample(torch.zeros(4096), 48000, 44100, **KAISER_BEST)
    x = torch.zeros(2, 100)
    assert Resample(44100, 44100)(x) is x and Resample()(x) is x and Resample(96000, 96000, **KAISER_BEST)(x) is x
    assert RS.resample(x, 16000, 16000) is x
    with pytest.raises(ValueError, match="resampling_method"):
        Resample(48000, 44100, resampling_method="linear")
    with pytest.raises(ValueError):
        Resample(0, 44100)


def test_read_wav_rate_and_the_default_wav2spec(tmp_path):
    rng = np.random.default_rng(2)
    x = np.round(rng.uniform(-1, 1, (500, 1)) * 32768).clip(-32768, 32767) / 32768
    p = str(tmp_path / "r22.wav")
    write_wav(p, x, 22050, 1, 16)
    got, sr = M.read_wav_rate(p)
    assert sr == 22050 and got.dtype == np.float32
    np.testing.assert_array_equal(got, x[:, 0].astype(np.float32))
    np.testing.assert_array_equal(M.read_wav(p), got)
    hp = dict(audio_sample_rate=44100, audio_num_mel_bins=128, fft_size=2048, win_size=2048, hop_size=512, fmin=40,
              fmax=16000)
    with pytest.raises(ValueError, match="no resampler"):
        NsfHifiGAN.wav2spec(p, hp)
