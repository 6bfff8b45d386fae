"""float64 restatement of the reference's mel analysis, modules/nsf_hifigan/nvSTFT.py:48-98 (STFT.get_mel), in
numpy, and the fixture cases of tests/golden/gen_golden_mel.py.

    :58-61  factor = 2^(keyshift/12); n_fft_new, win_size_new = round(. * factor); hop_length_new = round(hop * speed)
    :75     torch.hann_window(win_size_new)            periodic Hann, here in float64 (the reference's is float32)
    :77-80  reflect pad (win_new - hop_new)//2 left, (win_new - hop_new + 1)//2 right
    :82-87  torch.stft(center=False, win_length < n_fft: the window is zero-padded on both sides, centred).abs()
    :88-93  keyshift != 0: zero-pad or cut the bins to n_fft//2 + 1, times win_size / win_size_new
    :95     mel_basis @ spec                           the basis is data (float32 values, summed in float64)
    :96     log(clamp(., min=clip_val))                dynamic_range_compression_torch :25-26, C = 1
"""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

SVS = dict(sr=44100, n_mels=128, n_fft=2048, win_size=2048, hop_length=512, fmin=40, fmax=16000)
TTS = dict(sr=22050, n_mels=80, n_fft=1024, win_size=1024, hop_length=256, fmin=20, fmax=11025)
SHORT_WIN = dict(sr=22050, n_mels=80, n_fft=1024, win_size=800, hop_length=200, fmin=20, fmax=11025)

# name -> (STFT settings, keyshift, speed, L, one signal kind per batch row)
CASES = {
    "base": (SVS, 0, 1, 12 * 512 + 37, ("noise", "harmonic")),       # the trailing partial hop is dropped
    "ks7": (SVS, 7, 1, 12 * 512 + 37, ("harmonic", "noise")),        # nf 3069, odd; bins cut to 1025
    "ksm7": (SVS, -7, 1, 12 * 512 + 37, ("quiet", "noise")),         # nf 1367, odd; bins 684..1024 zero
    "ks12": (SVS, 12, 1, 12 * 512 + 37, ("harmonic",)),              # nf 4096
    "ksm12": (SVS, -12, 1, 12 * 512 + 37, ("noise", "quiet")),       # nf 1024
    "speed125": (SVS, 0, 1.25, 12 * 512 + 37, ("harmonic", "noise")),   # hop 640
    "ks3_speed08": (SVS, 3, 0.8, 12 * 512 + 37, ("noise", "harmonic")),  # nf 2435, hop 410
    "tts": (TTS, 0, 1, 12 * 256 + 19, ("harmonic", "noise")),
    "short_win": (SHORT_WIN, 0, 1, 12 * 200 + 19, ("noise", "quiet")),  # the window centred in the frame
    "shortest": (SVS, 0, 1, 769, ("noise",)),                        # the shortest legal signal, T = 1
    "t33": (SVS, 0, 1, 33 * 512, ("zeros", "quiet")),                # one frame over a 32-frame tile
    "t31": (SVS, 0, 1, 31 * 512, ("harmonic", "zeros")),             # one frame under
}


def derived_sizes(cfg, keyshift, speed):
    factor = 2 ** (keyshift / 12)
    return (int(np.round(cfg["n_fft"] * factor)), int(np.round(cfg["win_size"] * factor)),
            int(np.round(cfg["hop_length"] * speed)))


def num_frames(L, cfg, keyshift, speed):
    nf, wn, hn = derived_sizes(cfg, keyshift, speed)
    return 1 + (L + wn - hn - nf) // hn


def make_signal(kind, L, sr, seed):
    """Seeded test signals, no amplitude above 1."""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.uniform(-1.0, 1.0, L).astype(np.float32)
    t = np.arange(L) / sr
    f0 = 220.0 * (1.0 + 0.02 * np.sin(2 * np.pi * 5.5 * t))           # vibrato
    ph = 2 * np.pi * np.cumsum(f0) / sr
    x = sum(np.sin(k * ph + rng.uniform(0, 2 * np.pi)) / k for k in range(1, 31))
    x = 0.8 * x / np.abs(x).max() + 0.003 * rng.uniform(-1.0, 1.0, L)
    if kind == "quiet":
        x[L // 3:2 * L // 3] *= 1e-4                                   # a quiet middle third
    elif kind == "zeros":
        x[L // 4:L // 4 + 3 * 2048] = 0.0                              # exact zeros over several frames: the clip
    else:
        assert kind == "harmonic", kind
    return x.astype(np.float32)


def case_wav(name):
    cfg, _, _, L, kinds = CASES[name]
    seed0 = sorted(CASES).index(name) * 16
    return np.stack([make_signal(k, L, cfg["sr"], seed0 + i) for i, k in enumerate(kinds)])


def get_mel64(y, basis, cfg, keyshift=0, speed=1, clip_val=1e-5):
    """y [B, L], basis [n_mels, n_fft//2 + 1] -> (log-mel [B, n_mels, T], magnitude [B, n_fft//2 + 1, T],
    l1 [B, 1, T] = sum_n |y[n]| over each frame, on the magnitude's scale: what bounds a float32 DFT's
    rounding error, the absolute rounding of a float32 window included), float64 throughout."""
    y = np.asarray(y, np.float64)
    n_fft, win_size = cfg["n_fft"], cfg["win_size"]
    nf, wn, hn = derived_sizes(cfg, keyshift, speed)
    yp = np.pad(y, ((0, 0), ((wn - hn) // 2, (wn - hn + 1) // 2)), mode="reflect")
    T = 1 + (yp.shape[1] - nf) // hn
    win = np.zeros(nf)
    left = (nf - wn) // 2
    win[left:left + wn] = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(wn) / wn)
    frames = np.stack([yp[:, t * hn:t * hn + nf] for t in range(T)], axis=1)      # [B, T, nf]
    spec = np.abs(np.fft.rfft(frames * win, axis=-1)).transpose(0, 2, 1)          # [B, nf//2 + 1, T]
    l1 = np.abs(frames).sum(axis=-1)[:, None, :]
    if keyshift != 0:
        size = n_fft // 2 + 1
        if spec.shape[1] < size:
            spec = np.pad(spec, ((0, 0), (0, size - spec.shape[1]), (0, 0)))
        spec = spec[:, :size] * win_size / wn
        l1 = l1 * win_size / wn
    mel = np.einsum("mk,bkt->bmt", np.asarray(basis, np.float64), spec)
    return np.log(np.maximum(mel, clip_val)), spec, l1


@functools.lru_cache(maxsize=None)
def fixture(name):
    """tests/golden/mel_<name>.npz; shared by the tests, not to be written to."""
    with np.load(os.path.join(GOLDEN, f"mel_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def restated(name):
    """get_mel64 of a fixture's wav with the fixture's basis, computed once per session."""
    cfg, keyshift, speed, _, _ = CASES[name]
    d = fixture(name)
    return get_mel64(d["wav"], d["basis"], cfg, keyshift, speed)
