"""The float64 definition of the polyphase windowed-sinc resampler (what torchaudio.functional.resample
computes: padding (W, W + o), conv1d with stride o, truncation), written out independently of
prodiff_amd/resample.py; its restatement as one scipy.signal.upfirdn call; and the case table the CPU and GPU
tests share."""
from fractions import Fraction
from math import ceil, gcd, pi

import numpy as np

BETA = 14.769656459379492
KAISER_BEST = dict(lowpass_filter_width=64, rolloff=0.9475937167399596, resampling_method="sinc_interp_kaiser",
                   beta=BETA)
HANN, KAISER = "sinc_interp_hann", "sinc_interp_kaiser"

# name -> (orig, new, keyword arguments, (o, n, W, K) or None)
CASES = {
    "a": (48000, 44100, dict(resampling_method=HANN, lowpass_filter_width=6), (160, 147, 7, 174)),
    "b": (44100, 16000, dict(resampling_method=HANN, lowpass_filter_width=128), (441, 160, 357, 1155)),
    "c": (22050, 44100, dict(resampling_method=HANN, lowpass_filter_width=6), (1, 2, 7, 15)),
    "d": (48000, 16000, dict(resampling_method=KAISER, lowpass_filter_width=6), (3, 1, 19, 41)),
    "e": (44100, 48000, dict(KAISER_BEST), None),
    "f": (32000, 44100, dict(resampling_method=KAISER, lowpass_filter_width=16), (320, 441, 17, 354)),
}


def reduced(orig, new):
    g = gcd(orig, new)
    return orig // g, new // g


def group(n):
    """Frames the kernel treats as one: G = ceil(32 / n)."""
    return -(-32 // n)


def table64(orig, new, lowpass_filter_width=6, rolloff=0.99, resampling_method=HANN, beta=None):
    """(h float64 [n][K], W, o, n), entry by entry as the definition states it."""
    o, n = reduced(orig, new)
    lw = lowpass_filter_width
    base = min(o, n) * rolloff
    W = int(ceil(lw * o / base))
    K = 2 * W + o
    b = BETA if beta is None else beta
    t = np.empty((n, K))
    for p in range(n):
        for k in range(K):
            t[p, k] = ((k - W) / o - p / n) * base
    t = np.minimum(np.maximum(t, -lw), lw)
    if resampling_method == HANN:
        w = np.square(np.cos(t * pi / lw / 2))
    elif resampling_method == KAISER:
        w = np.i0(b * np.sqrt(1 - np.square(t / lw))) / np.i0(b)
    else:
        raise ValueError(resampling_method)
    return np.sinc(t) * w * (base / o), W, o, n       # np.sinc(t) = sin(pi t) / (pi t), 1 at 0


def out_len(L, o, n):
    return int(ceil(Fraction(n * L, o)))


def windows(x, h, W, o, n):
    """[Q][K] input windows of the rows of float64 x [B][L] (zero outside), Q = ceil(len / n) frames."""
    B, L = x.shape
    Q = -(-out_len(L, o, n) // n)
    K = h.shape[1]
    xp = np.zeros((B, W + (Q - 1) * o + K + L))
    xp[:, W:W + L] = x
    idx = (np.arange(Q) * o)[:, None] + np.arange(K)[None, :]
    return xp[:, idx]                                  # [B][Q][K]: x[q o + k - W]


def direct64(x, h, W, o, n):
    """y[q n + p] = sum_k h[p][k] x[q o + k - W] in float64 -> [B][ceil(n L / o)]."""
    x = np.atleast_2d(np.asarray(x, np.float64))
    win = windows(x, h, W, o, n)
    y = np.einsum("bqk,pk->bqp", win, h).reshape(x.shape[0], -1)
    return y[:, :out_len(x.shape[1], o, n)]


def abs_sum64(x, h32, W, o, n):
    """sum_k |h[p][k]| |x[q o + k - W]| per output sample, the scale of the fma chain's rounding bound."""
    x = np.atleast_2d(np.asarray(x, np.float64))
    win = np.abs(windows(x, h32, W, o, n))
    s = np.einsum("bqk,pk->bqp", win, np.abs(np.asarray(h32, np.float64))).reshape(x.shape[0], -1)
    return s[:, :out_len(x.shape[1], o, n)]


def upfirdn_prototype(h, W, o, n):
    """(G, first): scipy.signal.upfirdn(G, x, up=n, down=o)[first:] is the resampler's output:
    G[p o - k n + W n + D] = h[p][k], D the smallest multiple of o that is >= (W + o - 1) n, first = D / o."""
    K = h.shape[1]
    D = -(-(W + o - 1) * n // o) * o
    G = np.zeros((n - 1) * o + W * n + D + 1)
    for p in range(n):
        for k in range(K):
            G[p * o - k * n + W * n + D] = h[p, k]
    return G, D // o


def upfirdn64(x, h, W, o, n):
    from scipy.signal import upfirdn
    G, first = upfirdn_prototype(h, W, o, n)
    x = np.asarray(x, np.float64)
    y = upfirdn(G, x, up=n, down=o)
    m = out_len(len(x), o, n)
    y = y[first:first + m]
    return np.concatenate([y, np.zeros(m - len(y))])
