"""Mel-spectrogram analysis on the GPU: the reference's modules/nsf_hifigan/nvSTFT.py (``STFT.get_mel``)
on pd_mel (include/prodiff_hip.h), and the Slaney mel filterbank that ``librosa.filters.mel`` builds with
its defaults (nvSTFT.py:70), restated here so that no librosa is needed.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib


# ---------------------------------------------------------------- filterbank
_F_SP = 200.0 / 3            # Hz per mel below the knee
_MIN_LOG_HZ = 1000.0         # the knee: linear below, logarithmic above
_MIN_LOG_MEL = _MIN_LOG_HZ / _F_SP
_LOGSTEP = np.log(6.4) / 27.0


def hz_to_mel(f):
    """Slaney's Auditory Toolbox scale (librosa's default, htk=False)."""
    f = np.asarray(f, np.float64)
    return np.where(f >= _MIN_LOG_HZ, _MIN_LOG_MEL + np.log(np.maximum(f, 1e-300) / _MIN_LOG_HZ) / _LOGSTEP, f / _F_SP)


def mel_to_hz(m):
    m = np.asarray(m, np.float64)
    return np.where(m >= _MIN_LOG_MEL, _MIN_LOG_HZ * np.exp(_LOGSTEP * (m - _MIN_LOG_MEL)), _F_SP * m)


def hz_to_mel_htk(f):
    """The HTK scale (librosa's htk=True): mel = 2595 log10(1 + f / 700)."""
    return 2595.0 * np.log10(1.0 + np.asarray(f, np.float64) / 700.0)


def mel_to_hz_htk(m):
    return 700.0 * (10.0 ** (np.asarray(m, np.float64) / 2595.0) - 1.0)


def mel_filterbank64(sr, n_fft, n_mels, fmin=0.0, fmax=None, htk=False):
    """float64 [n_mels, n_fft // 2 + 1]: triangles between n_mels + 2 points equally spaced on the Slaney
    scale (the HTK scale with ``htk``) from fmin to fmax (sr / 2 when None), each scaled by 2 / (its base in
    Hz) -- Slaney's area normalisation: every triangle has unit area over frequency."""
    fmax = sr / 2.0 if fmax is None else float(fmax)
    freqs = np.linspace(0.0, sr / 2.0, 1 + n_fft // 2)
    if htk:
        pts = mel_to_hz_htk(np.linspace(hz_to_mel_htk(fmin), hz_to_mel_htk(fmax), n_mels + 2))
    else:
        pts = mel_to_hz(np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), n_mels + 2))
    width = np.diff(pts)
    ramps = pts[:, None] - freqs[None, :]
    lower = -ramps[:-2] / width[:-1, None]
    upper = ramps[2:] / width[1:, None]
    w = np.maximum(0.0, np.minimum(lower, upper))
    return w * (2.0 / (pts[2:] - pts[:-2]))[:, None]


def mel_filterbank(sr, n_fft, n_mels, fmin=0.0, fmax=None, htk=False):
    """``librosa.filters.mel(sr=, n_fft=, n_mels=, fmin=, fmax=, htk=)`` with its other defaults (Slaney
    norm; Slaney scale unless ``htk``): computed in float64, returned as float32 [n_mels, n_fft // 2 + 1]."""
    return mel_filterbank64(sr, n_fft, n_mels, fmin, fmax, htk).astype(np.float32)


# ---------------------------------------------------------------- native front end
def derived_sizes(n_fft, win_size, hop_length, keyshift=0, speed=1):
    """(nf, wn, hn): frame, window and hop in samples (nvSTFT.py:58-61)."""
    factor = 2 ** (keyshift / 12)
    return (int(np.round(n_fft * factor)), int(np.round(win_size * factor)), int(np.round(hop_length * speed)))


def num_frames(n_samples, n_fft, win_size, hop_length, keyshift=0, speed=1):
    """Frames ``get_mel`` returns for a signal of n_samples (center=False on the reflect-padded signal)."""
    nf, wn, hn = derived_sizes(n_fft, win_size, hop_length, keyshift, speed)
    return 1 + (n_samples + wn - hn - nf) // hn


class MelFrontEnd:
    """What ``STFT`` and ``rmvpe.MelSpectrogram`` share: the filterbank on each device, up to eight pd_mel handles
    in total (one per key shift, speed and device, oldest out first) and the pd_mel_forward call.  A subclass names
    its create function and states its minimum-length rule (``_min_samples``)."""

    def _setup(self, name, create, basis, n_fft, win_size, hop_length, clip_val, create_extra=()):
        self._sizes = (n_fft, win_size, hop_length, basis.shape[0])
        self._clip = float(clip_val)
        self.mel_basis_host = torch.from_numpy(np.ascontiguousarray(basis))
        self.mel_basis = {}      # device -> tensor
        # like the reference's window / basis dicts
        self._cache = _lib.HandleCache(name, create, "pd_mel_destroy", limit=8, create_extra=create_extra)
        self.handles = self._cache.handles      # (keyshift, speed, device) -> NativeHandle

    def handle(self, keyshift, speed, device):
        def build(device):
            basis = self.mel_basis.get(str(device))
            if basis is None:
                basis = self.mel_basis[str(device)] = self.mel_basis_host.to(device)
            return _lib.pd_mel_dims(*self._sizes, float(keyshift), float(speed), self._clip), [basis]
        return self._cache.get(device, (float(keyshift), float(speed)), build)

    def close(self):
        self._cache.close()

    def _min_samples(self, keyshift, speed):
        """(shortest legal signal, what needs it: the tail of the error text)."""
        raise NotImplementedError

    @torch.no_grad()
    def _mel_time_major(self, y, keyshift, speed, lens=None, out_scale=1.0, return_spec=False):
        if y.dim() == 1:
            y = y[None]
        y = y.float().contiguous()
        B, L = y.shape
        need, why = self._min_samples(keyshift, speed)
        if L < need:
            raise ValueError(f"signal of {L} samples is too short: {why} at least {need}")
        dev = y.device
        h = self.handle(keyshift, speed, dev)
        lib = _lib.lib()
        T = lib.pd_mel_frames(h, L)
        ln = None
        if lens is not None:
            ln = _lib._device_rows(lens, B, dev, "lens", need, L)
        n_mels, n_bins = self.mel_basis_host.shape
        out = torch.empty(B, T, n_mels, device=dev, dtype=torch.float32)
        spec = torch.empty(B, T, n_bins, device=dev, dtype=torch.float32) if return_spec else None
        # pd_mel_workspace_size is 0: the kernel keeps everything in LDS and registers
        _lib.check(lib.pd_mel_forward(h, _lib.fptr(y), _lib.iptr(ln), float(out_scale), _lib.fptr(out), _lib.fptr(spec),
                                      B, L, None, 0, _lib.stream_ptr(dev)))
        return (out, spec) if return_spec else out


class STFT(MelFrontEnd):
    """nvSTFT.py:33-98.  ``get_mel`` returns the reference's [B, n_mels, T]: a transposed view of the
    native time-major output, which ``get_mel_time_major`` returns as it is.  ``mel_basis`` (float
    [n_mels, n_fft // 2 + 1]) replaces the built-in Slaney filterbank, e.g. by librosa's own."""

    def __init__(self, sr=22050, n_mels=80, n_fft=1024, win_size=1024, hop_length=256, fmin=20, fmax=11025,
                 clip_val=1e-5, mel_basis=None):
        self.target_sr = sr
        self.n_mels, self.n_fft, self.win_size, self.hop_length = n_mels, n_fft, win_size, hop_length
        self.fmin, self.fmax, self.clip_val = fmin, fmax, clip_val
        basis = mel_filterbank(sr, n_fft, n_mels, fmin, fmax) if mel_basis is None else np.asarray(mel_basis, np.float32)
        if basis.shape != (n_mels, n_fft // 2 + 1):
            raise ValueError(f"mel_basis must be [{n_mels}, {n_fft // 2 + 1}], got {basis.shape}")
        self._setup("STFT.get_mel", "pd_mel_create", basis, n_fft, win_size, hop_length, clip_val)

    def min_samples(self, keyshift=0, speed=1):
        nf, wn, hn = derived_sizes(self.n_fft, self.win_size, self.hop_length, keyshift, speed)
        return max((wn - hn + 1) // 2 + 1, nf - wn + hn)

    def _min_samples(self, keyshift, speed):
        return self.min_samples(keyshift, speed), f"keyshift {keyshift}, speed {speed} need"

    def get_mel_time_major(self, y, keyshift=0, speed=1, center=False, lens=None, out_scale=1.0, return_spec=False):
        """y [B, L] (or [L]) on the GPU -> natural-log mel [B, T, n_mels] times ``out_scale``; with
        ``return_spec`` also the magnitude spectrum [B, T, n_fft // 2 + 1].  ``lens``: samples per row of a
        ragged batch (frames past a row's own count are unspecified)."""
        if center:
            raise NotImplementedError("center=True is not offered (the reference's callers use center=False)")
        return self._mel_time_major(y, keyshift, speed, lens, out_scale, return_spec)

    def get_mel(self, y, keyshift=0, speed=1, center=False, lens=None):
        """nvSTFT.py:48-98: y [B, L] -> [B, n_mels, T] natural-log mel."""
        return self.get_mel_time_major(y, keyshift, speed, center, lens).transpose(1, 2)

    def __call__(self, audiopath):
        """nvSTFT.py:100-103: a WAV file at the STFT's rate -> [n_mels, T]."""
        wav = torch.from_numpy(read_wav(audiopath, self.target_sr)).cuda()
        return self.get_mel(wav[None])[0]


# ---------------------------------------------------------------- WAV files
def read_wav(path, expect_sr=None):
    """A PCM16 / PCM32 / float32 RIFF WAV, mono or multi-channel -> float32 [n] in [-1, 1), channels
    averaged.  ``expect_sr``: raise if the file's rate differs (there is no resampler here: read_wav_rate
    returns the file's rate, prodiff_amd.resample converts)."""
    return _read_wav(path, expect_sr)[0]


def read_wav_rate(path):
    """``read_wav`` of a file at any rate -> (float32 [n], sample_rate)."""
    return _read_wav(path, None)


def _read_wav(path, expect_sr):
    import struct
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"WAVE":
        raise ValueError(f"{path}: not a RIFF/WAVE file")
    pos, fmt, pcm = 12, None, None
    while pos + 8 <= len(data):
        cid, size = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
        body = data[pos + 8:pos + 8 + size]
        if cid == b"fmt ":
            fmt = struct.unpack("<HHIIHH", body[:16])
            if fmt[0] == 0xFFFE and len(body) >= 26:     # WAVE_FORMAT_EXTENSIBLE: the sub-format's first two bytes
                fmt = (struct.unpack("<H", body[24:26])[0],) + fmt[1:]
        elif cid == b"data":
            pcm = body
        pos += 8 + size + (size & 1)
    if fmt is None or pcm is None:
        raise ValueError(f"{path}: no fmt / data chunk")
    tag, channels, sr, _, _, bits = fmt
    if expect_sr is not None and sr != int(expect_sr):
        raise ValueError(f"{path}: sample rate {sr} differs from audio_sample_rate {int(expect_sr)} "
                         "(resample the file first: there is no resampler here)")
    if tag == 1 and bits == 16:
        x = np.frombuffer(pcm[:len(pcm) // 2 * 2], "<i2").astype(np.float32) / 32768.0
    elif tag == 1 and bits == 32:
        x = (np.frombuffer(pcm[:len(pcm) // 4 * 4], "<i4").astype(np.float64) / 2147483648.0).astype(np.float32)
    elif tag == 3 and bits == 32:
        x = np.frombuffer(pcm[:len(pcm) // 4 * 4], "<f4").astype(np.float32)
    else:
        raise ValueError(f"{path}: unsupported WAV format (tag {tag}, {bits} bits); PCM16, PCM32 and float32 are read")
    if channels < 1:
        raise ValueError(f"{path}: no channels")
    x = x[:len(x) // channels * channels].reshape(-1, channels)
    return np.ascontiguousarray(x.mean(axis=1, dtype=np.float64).astype(np.float32) if channels > 1 else x[:, 0]), int(sr)
