"""float64 restatement of the reference's FastDiff analysis, utils/data_gen_utils.py:95-149 (process_utterance), with
what it calls in pyloudnorm (Meter.integrated_loudness, normalize.loudness), librosa 0.8 (stft, filters.mel) and
utils/audio.py (librosa_pad_lr, amp_to_db, normalize), in numpy and scipy; and the fixture cases of
tests/golden/gen_golden_analysis.py.

    pyloudnorm  K-weighting: high shelf (G 4 dB, Q 1/sqrt 2, fc 1500 Hz), high pass (Q 0.5, fc 38 Hz), each
                scipy.signal.lfilter(b, a, x); blocks of 0.4 s at 75 % overlap with bounds int(0.4 (j 0.25) rate),
                int(0.4 (j 0.25 + 1) rate), int(round((T - 0.4) / 0.1) + 1) of them; z_j = sum y^2 / (0.4 rate);
                l_j = -0.691 + 10 log10 z_j; gates l_j >= -70, then l_j > Gamma_r and l_j > -70
    :120-122    gain = 10^((-22 - L) / 20) applied in float32 (the reference is numpy < 1.24 code: a float64
                scalar does not promote a float32 array), divided by the peak when that exceeds 1
    :125-127    librosa.stft(center=True, pad_mode="constant"): n_fft / 2 zeros on both sides, periodic Hann of
                win_length centred in n_fft, T = 1 + L // hop
    :132-136    mel = basis @ |X|; log10(max(eps, mel)) for vocoder == 'pwg' only
    :140-142    the waveform right-padded with zeros and cut to T hop
    :147-148    spc = (20 log10(max(1e-5, |X|)) - min_level_db) / -min_level_db
"""
import functools
import os

import numpy as np
from scipy.signal import lfilter

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

TTS = dict(sample_rate=22050, fft_size=1024, hop_size=256, win_length=1024, num_mels=80, fmin=80, fmax=7600)
CHUNK = 512          # pd_loudness_chunk(): the fixtures' lengths are placed around its multiples
GATE_MARGIN = 0.01   # dB: no block of any fixture lies this close to either gate

# name -> (rate, L, kind)
LOUD_CASES = {
    "r16_045": (16000, 7200, "noise"),            # 0.45 s
    "r22_045": (22050, 9922, "harmonic"),         # 0.45 s
    "r16_075": (16000, 12000, "harmonic"),        # 0.75 s
    "r22_075": (22050, 16537, "noise"),           # 0.75 s
    "r16_130": (16000, 20800, "noise"),           # 1.3 s
    "r22_130": (22050, 28665, "harmonic"),        # 1.3 s, no multiple of the chunk
    "chunk_x20": (22050, 20 * CHUNK, "noise"),    # a whole number of chunks
    "chunk_x20m1": (22050, 20 * CHUNK - 1, "noise"),   # one sample short of a chunk boundary
    "gate": (16000, 48000, "gate"),               # loud, exact zeros, 20 dB down: both gates bite
    "clicks": (22050, 14000, "clicks"),           # quiet with sparse peaks: the gain drives it past 1.0
}
MEL_CASES = ("r22_130", "clicks", "r22_045")      # process_utterance at TTS dims


def make_signal(kind, L, rate, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(L) / rate
    if kind == "noise":
        return (0.5 * rng.uniform(-1.0, 1.0, L)).astype(np.float32)
    f0 = 180.0 * (1.0 + 0.03 * np.sin(2 * np.pi * 4.5 * t))
    ph = 2 * np.pi * np.cumsum(f0) / rate
    x = sum(np.sin(k * ph + rng.uniform(0, 2 * np.pi)) / k for k in range(1, 21))
    x = 0.6 * x / np.abs(x).max() + 0.002 * rng.uniform(-1.0, 1.0, L)
    if kind == "gate":
        a, b = int(0.4 * L), int(0.65 * L)
        x[a:b] = 0.0                              # exact zeros: blocks inside fall to the absolute gate
        x[b:] *= 0.1                              # 20 dB down: blocks inside fall to the relative gate
    elif kind == "clicks":
        x *= 0.004
        x[::1733] = 0.9 * np.sign(rng.uniform(-1, 1, x[::1733].shape))
    else:
        assert kind == "harmonic", kind
    return x.astype(np.float32)


def case_wav(name):
    rate, L, kind = LOUD_CASES[name]
    return make_signal(kind, L, rate, 4000 + sorted(LOUD_CASES).index(name))


# ---------------------------------------------------------------- BS.1770
def k_filters(rate):
    """[(b, a)] of the two stages, a[0] = 1: the audio-EQ-cookbook high shelf and high pass as pyloudnorm writes them."""
    def shelf(G, Q, fc):
        A = 10 ** (G / 40.0)
        w0 = 2.0 * np.pi * (fc / rate)
        al = np.sin(w0) / (2.0 * Q)
        c, r = np.cos(w0), 2 * np.sqrt(A) * al
        b = np.array([A * ((A + 1) + (A - 1) * c + r), -2 * A * ((A - 1) + (A + 1) * c), A * ((A + 1) + (A - 1) * c - r)])
        a = np.array([(A + 1) - (A - 1) * c + r, 2 * ((A - 1) - (A + 1) * c), (A + 1) - (A - 1) * c - r])
        return b / a[0], a / a[0]

    def high_pass(Q, fc):
        w0 = 2.0 * np.pi * (fc / rate)
        al = np.sin(w0) / (2.0 * Q)
        c = np.cos(w0)
        b = np.array([(1 + c) / 2, -(1 + c), (1 + c) / 2])
        a = np.array([1 + al, -2 * c, 1 - al])
        return b / a[0], a / a[0]
    return [shelf(4.0, 1 / np.sqrt(2), 1500.0), high_pass(0.5, 38.0)]


def blocks(L, rate):
    """[(l_j, u_j)] as pyloudnorm evaluates them."""
    T = L / rate
    n = int(np.round(((T - 0.4) / (0.4 * 0.25))) + 1)
    return [(int(0.4 * (j * 0.25) * rate), int(0.4 * (j * 0.25 + 1) * rate)) for j in range(n)]


def loudness_detail(x, rate):
    """-> dict(loud, z [n], l [n], gamma_r, abs_gate [n] bool, rel_gate [n] bool)."""
    x = np.asarray(x, np.float64)
    if x.shape[0] < 0.4 * rate:
        raise ValueError("Audio must have length greater than the block size.")
    y = x
    for b, a in k_filters(rate):
        y = lfilter(b, a, y)
    z = np.array([(1.0 / (0.4 * rate)) * np.sum(np.square(y[l:u])) for l, u in blocks(len(x), rate)])
    with np.errstate(divide="ignore", invalid="ignore"):
        lj = -0.691 + 10.0 * np.log10(z)
        ga = lj >= -70.0
        gamma_r = -0.691 + 10.0 * np.log10(np.mean(z[ga]) if ga.any() else np.nan) - 10.0
        gr = (lj > gamma_r) & (lj > -70.0)
        loud = -0.691 + 10.0 * np.log10(np.mean(z[gr]) if gr.any() else 0.0)
    return dict(loud=float(loud), z=z, l=lj, gamma_r=float(gamma_r), abs_gate=ga, rel_gate=gr)


def integrated_loudness64(x, rate):
    return loudness_detail(x, rate)["loud"]


def gate_margin(d):
    """The smallest distance in dB of any block's l_j from -70 and from Gamma_r (inf for silent blocks)."""
    lj = d["l"][np.isfinite(d["l"])]
    m = np.abs(lj + 70.0).min() if lj.size else np.inf
    if np.isfinite(d["gamma_r"]) and lj.size:
        m = min(m, np.abs(lj - d["gamma_r"]).min())
    return float(m)


def normalize32(x, loud, target=-22.0):
    """normalize.loudness, then :121-122, in float32 -> (wav float32, whether the peak branch was taken)."""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore"):
        g = np.float32(np.power(10.0, (target - loud) / 20.0))
    y = (g * x).astype(np.float32)
    peak = np.abs(y).max()
    if peak > 1:
        return (y / peak).astype(np.float32), True
    return y, False


# ---------------------------------------------------------------- STFT, mel
def hz_to_mel(f):
    f = np.asarray(f, np.float64)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0), f / (200.0 / 3))


def mel_to_hz(m):
    m = np.asarray(m, np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), (200.0 / 3) * m)


def mel_basis32(sr, n_fft, n_mels, fmin, fmax):
    """librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax): Slaney scale and norm, float32."""
    freqs = np.linspace(0.0, sr / 2.0, 1 + n_fft // 2)
    pts = mel_to_hz(np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), n_mels + 2))
    ramps = pts[:, None] - freqs[None, :]
    w = np.maximum(0.0, np.minimum(-ramps[:-2] / np.diff(pts)[:-1, None], ramps[2:] / np.diff(pts)[1:, None]))
    return (w * (2.0 / (pts[2:] - pts[:-2]))[:, None]).astype(np.float32)


def stft_mag64(x, n_fft, hop, win_length):
    """|librosa.stft(x, n_fft, hop, win_length, 'hann', center=True, pad_mode='constant')| -> [n_fft // 2 + 1, T]."""
    x = np.asarray(x, np.float64)
    xp = np.pad(x, (n_fft // 2, n_fft // 2), mode="constant")
    T = 1 + (len(xp) - n_fft) // hop
    win = np.zeros(n_fft)
    left = (n_fft - win_length) // 2
    win[left:left + win_length] = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(win_length) / win_length)
    frames = np.stack([xp[t * hop:t * hop + n_fft] for t in range(T)])
    return np.abs(np.fft.rfft(frames * win, axis=-1)).T


def process_utterance64(wav, fft_size=1024, hop_size=256, win_length=1024, num_mels=80, fmin=80, fmax=7600, eps=1e-6,
                        sample_rate=22050, loud_norm=False, min_level_db=-100, vocoder="pwg"):
    """-> dict(wav float32 [T hop], mel [num_mels, T], mag [bins, T], spc [bins, T], loud, peak_branch); the
    spectra in float64 from the float32 waveform the reference would hold."""
    wav = np.asarray(wav, np.float32)
    loud, took = None, False
    if loud_norm:
        loud = integrated_loudness64(wav, sample_rate)
        wav, took = normalize32(wav, loud, -22.0)
    mag = stft_mag64(wav, fft_size, hop_size, win_length)
    fmin = 0 if fmin == -1 else fmin
    fmax = sample_rate / 2 if fmax == -1 else fmax
    mel = mel_basis32(sample_rate, fft_size, num_mels, fmin, fmax).astype(np.float64) @ mag
    if vocoder == "pwg":
        mel = np.log10(np.maximum(eps, mel))
    pad = (wav.shape[0] // hop_size + 1) * hop_size - wav.shape[0]
    out = np.pad(wav, (0, pad), mode="constant")[:mel.shape[1] * hop_size]
    spc = (20 * np.log10(np.maximum(1e-5, mag)) - min_level_db) / -min_level_db
    return dict(wav=out, mel=mel, mag=mag, spc=spc, loud=loud, peak_branch=took)


# ---------------------------------------------------------------- fixtures
@functools.lru_cache(maxsize=None)
def fixture(name):
    """tests/golden/analysis_<name>.npz; shared by the tests, not to be written to."""
    with np.load(os.path.join(GOLDEN, f"analysis_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def detail(name):
    """loudness_detail of a fixture's wav, computed once per session."""
    return loudness_detail(fixture(name)["wav"], LOUD_CASES[name][0])


@functools.lru_cache(maxsize=None)
def restated(name, loud_norm, vocoder):
    """process_utterance64 of a fixture's wav at the TTS dims, computed once per session."""
    eps = 1e-6 if vocoder == "pwg" else 1e-10
    return process_utterance64(fixture(name)["wav"], loud_norm=loud_norm, vocoder=vocoder, eps=eps, **TTS)
