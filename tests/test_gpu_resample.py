"""GPU tests of the sample-rate conversion (pd_resample through prodiff_amd.resample.Resample and
NsfHifiGAN.wav2spec(resample=True)) against the float64 definition in tests/resample_ref.py.

The value bar is derived, not measured: an output is a K-step f32 fmaf chain over a table that was rounded once,
so it lies within (K + 2) 2^-24 sum_k |h[p][k]| |x[q o + k - W]| of the float64 sum (K roundings of the running
sum, each at most half an ulp of a partial sum that sum |h| |x| bounds, one for the table's rounding, one to
spare for the second-order terms); the bound is computed per output sample.
"""
import functools

import numpy as np
import pytest
import torch

from prodiff_amd import KAISER_BEST, STFT, Resample, _lib
from prodiff_amd.nsf_hifigan import NsfHifiGAN
from tests import resample_ref as R
from tests.test_mel_cpu import write_wav

pytestmark = pytest.mark.gpu

CASE_NAMES = sorted(R.CASES)
U = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def resampler(name):
    """One Resample per case for the whole session."""
    orig, new, kw, _ = R.CASES[name]
    return Resample(orig, new, **kw)


@functools.lru_cache(maxsize=None)
def table(name):
    orig, new, kw, _ = R.CASES[name]
    return R.table64(orig, new, **kw)


def cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def noise(seed, *shape):
    return np.random.default_rng(seed).uniform(-1, 1, shape).astype(np.float32)


def long_len(name):
    """33 regrouped frames and a bit: at least two blocks of 32."""
    h, W, o, n = table(name)
    return 33 * max(o, R.group(n) * o) + 5


def check_values(name, x, y):
    """y [B][M] float32 against the float64 direct sum of x [B][L]; returns the largest error / bound."""
    h, W, o, n = table(name)
    ref = R.direct64(x, h, W, o, n)
    bound = (h.shape[1] + 2) * U * R.abs_sum64(x, h.astype(np.float32), W, o, n)
    assert y.shape == ref.shape and np.isfinite(y).all()
    err = np.abs(y.astype(np.float64) - ref)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{name} L={x.shape[1]}: max err {err.max():.3e}, max err/bound {ratio:.3f}")
    assert (err <= bound).all(), (name, x.shape, ratio)
    return ratio


# ---------------------------------------------------------------- table
@pytest.mark.parametrize("name", CASE_NAMES)
def test_table_is_the_float64_table_rounded_once(name):
    h, W, o, n = table(name)
    r = resampler(name)
    assert (r.o, r.n, r.width) == (o, n, W)
    k = r.kernel
    assert k.dtype == torch.float32 and tuple(k.shape) == h.shape
    k = k.cpu().numpy().astype(np.float64)
    exp = np.maximum(np.frexp(np.abs(h))[1] - 1, -126)                    # floor(log2 |h|), f32's subnormal floor
    half_ulp = 0.5 * np.ldexp(1.0, exp - 23)
    d = np.abs(k - h)
    print(f"{name}: max |table - f64| / (half ulp + 1e-14) = {(d / (half_ulp + 1e-14)).max():.3f}")
    assert (d <= half_ulp + 1e-14).all()


# ---------------------------------------------------------------- values
@pytest.mark.parametrize("name", CASE_NAMES)
def test_values_within_the_fma_chain_bound(name):
    h, W, o, n = table(name)
    r = resampler(name)
    for i, L in enumerate((1, W, o + 1, long_len(name))):
        x = noise(100 * ord(name) + i, 2, L)
        y = r(cuda(x))
        assert tuple(y.shape) == (2, R.out_len(L, o, n)) and y.dtype == torch.float32
        check_values(name, x, y.cpu().numpy())
    one = r(cuda(x[0]))                                   # [L] -> [M], and the same numbers as in the batch
    assert one.dim() == 1 and torch.equal(one, y[0])
    three = r(cuda(x).reshape(2, 1, -1))                  # leading dimensions are kept
    assert tuple(three.shape) == (2, 1, y.shape[1]) and torch.equal(three[:, 0], y)


# ---------------------------------------------------------------- ragged batches
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_ragged_rows_equal_the_rows_alone(name):
    h, W, o, n = table(name)
    r = resampler(name)
    L = long_len(name)
    lens = [L, o + 1, 17 * o + 3]
    x = noise(7 + ord(name), 3, L)
    y = r(cuda(x), lens=lens)
    assert tuple(y.shape) == (3, R.out_len(L, o, n))
    for b, lb in enumerate(lens):
        alone = r(cuda(x[b:b + 1, :lb]))
        m = R.out_len(lb, o, n)
        assert tuple(alone.shape) == (1, m)
        assert torch.equal(y[b, :m], alone[0]), (name, b)
    y2 = r(cuda(x), lens=torch.tensor(lens, dtype=torch.int32, device="cuda"))      # device lens
    for b, lb in enumerate(lens):
        m = R.out_len(lb, o, n)
        assert torch.equal(y2[b, :m], y[b, :m])


# ---------------------------------------------------------------- tile position
@pytest.mark.parametrize("name", ["a", "c"])
def test_values_do_not_depend_on_the_tile_position(name):
    h, W, o, n = table(name)
    r = resampler(name)
    G = R.group(n)
    L = 70 * G * o + 3                                    # more than two blocks of 32 regrouped frames
    x = noise(11 + ord(name), 1, L)
    y = r(cuda(x))
    shifted = r(cuda(np.concatenate([np.zeros((1, 7 * G * o), np.float32), x], axis=1)))
    assert shifted.shape[1] == y.shape[1] + 7 * G * n
    assert torch.equal(shifted[:, 7 * G * n:], y)
    check_values(name, x, y.cpu().numpy())


# ---------------------------------------------------------------- lifecycle
def test_handle_lifecycle():
    lib = _lib.lib()
    torch.cuda.synchronize()
    before = lib.pd_live_device_bytes()
    r = Resample(48000, 44100, **KAISER_BEST)
    y = r(cuda(noise(3, 1, 1000)))
    assert y.shape[1] == R.out_len(1000, 160, 147)
    n, K = r.n, 2 * r.width + r.o
    assert lib.pd_live_device_bytes() >= before + 4 * n * K
    r.close()
    assert lib.pd_live_device_bytes() == before
    y2 = r(cuda(noise(3, 1, 1000)))                       # a closed Resample builds its handle again
    assert torch.equal(y, y2)
    r.close()
    assert lib.pd_live_device_bytes() == before


# ---------------------------------------------------------------- sine
def test_sine_comes_out_as_the_same_sine():
    """Case b (44.1 -> 16 kHz, width 128): the middle half of the output against the analytic sine at 16 kHz, within
    the float64 definition's own distance from it plus the fma chain's bound."""
    name = "b"
    h, W, o, n = table(name)
    f = 0.05 * 16000
    L = 40 * o + 8 * W
    x = np.sin(2 * np.pi * f * np.arange(L) / 44100).astype(np.float32)[None]
    y = resampler(name)(cuda(x)).cpu().numpy().astype(np.float64)
    ref = R.direct64(x, h, W, o, n)
    want = np.sin(2 * np.pi * f * np.arange(y.shape[1]) / 16000)[None]
    bound = (h.shape[1] + 2) * U * R.abs_sum64(x, h.astype(np.float32), W, o, n)
    mid = slice(y.shape[1] // 4, 3 * y.shape[1] // 4)
    e_ref = float(np.abs(ref - want)[:, mid].max())
    err = np.abs(y - want)[:, mid]
    print(f"sine: oracle {e_ref:.3e}, native {err.max():.3e}")
    assert (err <= e_ref + bound[:, mid]).all()


# ---------------------------------------------------------------- wav2spec(resample=True)
def test_wav2spec_resamples_a_48k_file(tmp_path):
    hp = dict(audio_sample_rate=44100, audio_num_mel_bins=128, fft_size=2048, win_size=2048, hop_size=512, fmin=40,
              fmax=16000)
    t = np.arange(24000)
    x = 0.5 * np.sin(2 * np.pi * 1000 * t / 48000)
    p = str(tmp_path / "sine48.wav")
    write_wav(p, x[:, None], 48000, 1, 16)
    with pytest.raises(ValueError, match="no resampler"):
        NsfHifiGAN.wav2spec(p, hp)
    wav, mel = NsfHifiGAN.wav2spec(p, hp, resample=True)
    pcm = (np.round(x * 32768).clip(-32768, 32767) / 32768).astype(np.float32)
    r = Resample(48000, 44100, **KAISER_BEST)
    s = STFT(44100, 128, 2048, 2048, 512, 40, 16000)
    try:
        y = r(cuda(pcm[None]))
        m = s.get_mel_time_major(y, out_scale=0.434294)[0]
        direct = 0.5 * np.sin(2 * np.pi * 1000 * np.arange(y.shape[1]) / 44100)
        md = s.get_mel_time_major(cuda(direct.astype(np.float32)[None]))[0].cpu().numpy()
        wav2, mel2 = NsfHifiGAN.wav2spec(pcm, hp, resample=True, orig_sr=48000)     # an array and its rate
    finally:
        r.close()
        s.close()
    assert wav.dtype == np.float32 and wav.shape == (22050,) and mel.shape == (m.shape[0], 128)
    np.testing.assert_array_equal(wav, y[0].cpu().numpy())
    np.testing.assert_array_equal(mel, m.cpu().numpy())
    np.testing.assert_array_equal(wav2, wav)
    np.testing.assert_array_equal(mel2, mel)
    T = mel.shape[0]
    mid = slice(T // 4, 3 * T // 4)
    np.testing.assert_array_equal(mel[mid].argmax(axis=1), md[mid].argmax(axis=1))
    same, _ = NsfHifiGAN.wav2spec(pcm, hp, resample=True)                          # no orig_sr: nothing to convert
    np.testing.assert_array_equal(same, pcm)
