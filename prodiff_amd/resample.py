"""Sample-rate conversion on the GPU: the polyphase windowed-sinc resampler that
``torchaudio.functional.resample`` defines, on pd_resample (include/prodiff_hip.h).  ``Resample`` takes the
arguments of ``torchaudio.transforms.Resample`` (the reference builds one in front of the RMVPE pitch
extractor, component/pe/rmvpe.py:49), ``resample`` is the functional form and ``KAISER_BEST`` the parameters
of the filter that utils/data_gen_utils.py:51 asks librosa for.  Neither torchaudio nor librosa is needed.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib

METHODS = {"sinc_interp_hann": 0, "sinc_interp_kaiser": 1}
DEFAULT_BETA = 14.769656459379492
# resampy's 'kaiser_best' design (64 zero crossings, rolloff 0.9476, Kaiser beta 14.77), as
# torchaudio's documentation maps it onto these arguments
KAISER_BEST = dict(lowpass_filter_width=64, rolloff=0.9475937167399596, resampling_method="sinc_interp_kaiser",
                   beta=14.769656459379492)


def sinc_resample_kernel64(orig, new, lowpass_filter_width=6, rolloff=0.99, resampling_method="sinc_interp_hann",
                           beta=None):
    """(h float64 [n, K], W, o, n): the table of n phase filters of K = 2 W + o taps each, with
    o = orig / gcd, n = new / gcd.  Output sample q n + p is sum_k h[p][k] x[q o + k - W]."""
    orig, new, width = int(orig), int(new), int(lowpass_filter_width)
    if orig <= 0 or new <= 0 or width <= 0:
        raise ValueError("orig_freq, new_freq and lowpass_filter_width must be positive")
    if resampling_method not in METHODS:
        raise ValueError(f"resampling_method must be one of {sorted(METHODS)}, got {resampling_method!r}")
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    base = min(o, n) * rolloff
    W = int(math.ceil(width * o / base))
    k = np.arange(-W, W + o, dtype=np.float64)[None, :] / o
    p = np.arange(0, -n, -1, dtype=np.float64)[:, None] / n
    t = np.clip((p + k) * base, -width, width)
    if resampling_method == "sinc_interp_hann":
        window = np.cos(t * math.pi / width / 2) ** 2
    else:
        b = DEFAULT_BETA if beta is None else float(beta)
        window = np.i0(b * np.sqrt(1 - (t / width) ** 2)) / np.i0(b)
    t = t * math.pi
    safe = np.where(t == 0, 1.0, t)
    h = np.where(t == 0, 1.0, np.sin(safe) / safe) * (window * (base / o))
    return h, W, o, n


class Resample:
    """``torchaudio.transforms.Resample``: ``Resample(orig, new)(waveform[..., L]) -> [..., ceil(new L / orig)]``
    on the GPU (a CPU tensor raises: there is no CPU fallback).  Equal rates return the input unchanged.
    ``lens``: samples per row of a ragged batch (a row's outputs past its own count are unspecified)."""

    def __init__(self, orig_freq=16000, new_freq=16000, resampling_method="sinc_interp_hann", lowpass_filter_width=6,
                 rolloff=0.99, beta=None):
        if resampling_method not in METHODS:
            raise ValueError(f"resampling_method must be one of {sorted(METHODS)}, got {resampling_method!r}")
        if int(orig_freq) != orig_freq or int(new_freq) != new_freq or orig_freq <= 0 or new_freq <= 0:
            raise ValueError("orig_freq and new_freq must be positive integers")
        if int(lowpass_filter_width) <= 0:
            raise ValueError("lowpass_filter_width must be positive")
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)
        self.resampling_method, self.lowpass_filter_width = resampling_method, int(lowpass_filter_width)
        self.rolloff, self.beta = float(rolloff), beta
        g = math.gcd(self.orig_freq, self.new_freq)
        self.o, self.n = self.orig_freq // g, self.new_freq // g
        self.width = int(math.ceil(self.lowpass_filter_width * self.o / (min(self.o, self.n) * self.rolloff)))
        self._cache = _lib.HandleCache("Resample", "pd_resample_create", "pd_resample_destroy")
        self.handles = self._cache.handles        # (device,) -> NativeHandle

    def _dims(self):
        return _lib.pd_resample_dims(self.orig_freq, self.new_freq, self.lowpass_filter_width, self.rolloff,
                                     METHODS[self.resampling_method], DEFAULT_BETA if self.beta is None else float(self.beta))

    def handle(self, device):
        return self._cache.get(device, (), lambda device: (self._dims(), []))

    def close(self):
        self._cache.close()

    def out_samples(self, n_samples):
        return -(-self.n * int(n_samples) // self.o)

    @property
    def kernel(self):
        """float32 [n, K] on the current device: the table as the kernel uses it (pd_resample_kernel)."""
        dev = torch.device("cuda", torch.cuda.current_device())
        h = self.handle(dev)
        lib = _lib.lib()
        o, n, W = C.c_int(), C.c_int(), C.c_int()
        _lib.check(lib.pd_resample_taps(h, C.byref(o), C.byref(n), C.byref(W)))
        if (o.value, n.value, W.value) != (self.o, self.n, self.width):
            raise _lib.HipError(f"pd_resample_taps {(o.value, n.value, W.value)} differ from {(self.o, self.n, self.width)}")
        out = torch.empty(self.n, 2 * self.width + self.o, device=dev, dtype=torch.float32)
        _lib.check(lib.pd_resample_kernel(h, _lib.fptr(out), _lib.stream_ptr(dev)))
        return out

    @torch.no_grad()
    def __call__(self, waveform, lens=None):
        if self.o == self.n:
            return waveform
        if not waveform.is_cuda:
            raise _lib.HipError("Resample runs on the GPU (got a CPU tensor; there is no CPU fallback)")
        shape = waveform.shape
        L = int(shape[-1])
        if L < 1 or L >= 2 ** 31:
            raise ValueError(f"the last dimension must hold 1 to 2^31 - 1 samples, got {L}")
        y = waveform.reshape(-1, L).float().contiguous()
        B, dev = y.shape[0], y.device
        h = self.handle(dev)
        lib = _lib.lib()
        ln = None if lens is None else _lib._device_rows(lens, B, dev, "lens", 0, L)
        out = torch.empty(B, self.out_samples(L), device=dev, dtype=torch.float32)
        for b0 in range(0, B, 65535):      # the batch is the grid's second dimension
            nb = min(B - b0, 65535)
            _lib.check(lib.pd_resample_forward(h, _lib.fptr(y[b0:b0 + nb]), _lib.iptr(None if ln is None else ln[b0:b0 + nb]),
                                               _lib.fptr(out[b0:b0 + nb]), nb, L, None, 0, _lib.stream_ptr(dev)))
        return out.reshape(*shape[:-1], out.shape[-1])

    forward = __call__


_CACHE = {}      # (rates, filter, device) -> Resample; at most eight, oldest out first


def resample(waveform, orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99, resampling_method="sinc_interp_hann",
             beta=None):
    """``torchaudio.functional.resample``.  The handles of the last eight (rate pair, filter, device) stay alive."""
    if int(orig_freq) == int(new_freq):
        return waveform
    key = (int(orig_freq), int(new_freq), int(lowpass_filter_width), float(rolloff), resampling_method, beta,
           str(waveform.device))
    r = _CACHE.get(key)
    if r is None:
        if len(_CACHE) >= 8:
            _CACHE.pop(next(iter(_CACHE))).close()
        r = _CACHE[key] = Resample(orig_freq, new_freq, resampling_method, lowpass_filter_width, rolloff, beta)
    return r(waveform)
