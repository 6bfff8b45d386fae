"""FastDiff's analysis half on the GPU: ``process_utterance`` of utils/data_gen_utils.py:95-149, which
component/vocoder/fastdiff.py:128-145 (``wav2spec``) calls, with the two libraries it leans on restated:

  * pyloudnorm's ``Meter(rate).integrated_loudness`` (ITU-R BS.1770: K-weighting, gated 400 ms blocks) and
    ``normalize.loudness`` on pd_loudness (include/prodiff_hip.h): the two biquads are designed here in float64
    from pyloudnorm's RBJ-style formulas, the block bounds are evaluated here in Python floats exactly as
    pyloudnorm writes them and uploaded as a table;
  * ``librosa.stft(center=True, pad_mode="constant")``, ``librosa.filters.mel`` and the magnitude-to-mel product on
    pd_mel_create_centered_zero.

Mono only.  ``trim_long_sil`` (webrtcvad) is not restated.
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from . import _lib
from .mel import MelFrontEnd, mel_filterbank, read_wav

BLOCK_SECONDS = 0.4          # T_g
TARGET_LUFS = -22.0          # process_utterance :120


# ---------------------------------------------------------------- K-weighting
def kweighting_coefficients(rate):
    """pyloudnorm's 'K-weighting' filter pair at ``rate``: {"shelf": (b, a), "pass": (b, a)}, float64 [3] each,
    a[0] = 1.  High shelf G = +4 dB, Q = 1/sqrt(2), fc = 1500 Hz; high pass Q = 0.5, fc = 38 Hz (its
    IIRfilter.generate_coefficients, the audio-EQ-cookbook forms)."""
    def design(kind, G, Q, fc):
        A = 10 ** (G / 40.0)
        w0 = 2.0 * np.pi * (fc / rate)
        alpha = np.sin(w0) / (2.0 * Q)
        if kind == "high_shelf":
            b0 = A * ((A + 1) + (A - 1) * np.cos(w0) + 2 * np.sqrt(A) * alpha)
            b1 = -2 * A * ((A - 1) + (A + 1) * np.cos(w0))
            b2 = A * ((A + 1) + (A - 1) * np.cos(w0) - 2 * np.sqrt(A) * alpha)
            a0 = (A + 1) - (A - 1) * np.cos(w0) + 2 * np.sqrt(A) * alpha
            a1 = 2 * ((A - 1) - (A + 1) * np.cos(w0))
            a2 = (A + 1) - (A - 1) * np.cos(w0) - 2 * np.sqrt(A) * alpha
        else:
            b0 = (1 + np.cos(w0)) / 2
            b1 = -(1 + np.cos(w0))
            b2 = (1 + np.cos(w0)) / 2
            a0 = 1 + alpha
            a1 = -2 * np.cos(w0)
            a2 = 1 - alpha
        return np.array([b0, b1, b2]) / a0, np.array([a0, a1, a2]) / a0
    return {"shelf": design("high_shelf", 4.0, 1 / np.sqrt(2), 1500.0), "pass": design("high_pass", 0.0, 0.5, 38.0)}


def block_count(n_samples, rate):
    """Blocks of a signal of n_samples: int(round((T - 0.4) / 0.1) + 1), T = n_samples / rate, in Python floats."""
    T = n_samples / rate
    return int(round((T - 0.4) / 0.1) + 1)


def block_bounds(rate, n_blocks):
    """[(l_j, u_j)] of the 400 ms blocks at 75 % overlap, in Python floats as pyloudnorm evaluates them; u_j may
    exceed the signal (the slice, and the kernel, stop at its end)."""
    return [(int(0.4 * (j * 0.25) * rate), int(0.4 * (j * 0.25 + 1) * rate)) for j in range(n_blocks)]


def min_samples(rate):
    """pyloudnorm refuses a signal shorter than one block (len < 0.4 rate)."""
    return int(math.ceil(BLOCK_SECONDS * rate))


def _check_lengths(lens, rate):
    for n in lens:
        if n < BLOCK_SECONDS * rate:
            raise ValueError(f"Audio must have length greater than the block size: {n} samples at {rate} Hz "
                             f"are shorter than one 400 ms block ({min_samples(rate)} samples)")


# ---------------------------------------------------------------- native meter
def _build_loudness(rate):
    k = kweighting_coefficients(rate)
    d = _lib.pd_loudness_dims()
    d.rate = int(rate)
    for name, vals in (("shelf_b", k["shelf"][0]), ("shelf_a", k["shelf"][1]), ("pass_b", k["pass"][0]),
                       ("pass_a", k["pass"][1])):
        setattr(d, name, (_lib.C.c_double * 3)(*[float(v) for v in vals]))
    return d, []


_METERS = _lib.HandleCache("loudness", "pd_loudness_create", "pd_loudness_destroy", limit=8)
_BOUNDS = {}                 # (rate, device) -> device int32 [n][2], grown as longer signals arrive
_WS = _lib.Workspace()


def _bounds_table(rate, n_blocks, dev):
    key = (int(rate), str(dev))
    t = _BOUNDS.get(key)
    if t is None or t.shape[0] < n_blocks:
        n = max(n_blocks, 64, 2 * (t.shape[0] if t is not None else 0))
        t = _BOUNDS[key] = torch.tensor(block_bounds(rate, n), dtype=torch.int32).to(dev)
    return t


def _as_batch(wav, lens, device):
    """wav: array / tensor [L] or [B, L] -> (float32 device [B, L], host lens [B], single)."""
    t = torch.as_tensor(wav) if not torch.is_tensor(wav) else wav
    single = t.dim() == 1
    if single:
        t = t[None]
    if t.dim() != 2:
        raise ValueError(f"wav must be [L] or [B, L] (mono), got {tuple(t.shape)}")
    B, L = t.shape
    if lens is None:
        host = [L] * B
    else:
        host = [int(v) for v in (lens.tolist() if torch.is_tensor(lens) else lens)]
        if len(host) != B or min(host) < 0 or max(host) > L:
            raise ValueError(f"lens must hold {B} values in [0, {L}]")
    return t, host, single


def _measure(y, host_lens, rate, target=None, L_out=None):
    """y float32 device [B, L] -> (loudness float64 [B], peak float32 [B], normalised wav [B, L_out] or None)."""
    B, L = y.shape
    dev = y.device
    h = _METERS.get(dev, (int(rate),), lambda d: _build_loudness(rate))
    lib = _lib.lib()
    counts = [block_count(n, rate) for n in host_lens]
    nb = max(counts)
    bounds = _bounds_table(rate, nb, dev)
    cnt = _lib._device_rows(counts, B, dev, "loudness blocks", 1, nb)
    ln = None if all(n == L for n in host_lens) else _lib._device_rows(host_lens, B, dev, "lens", min_samples(rate), L)
    loud = torch.empty(B, device=dev, dtype=torch.float64)
    peak = torch.empty(B, device=dev, dtype=torch.float32)
    out = torch.empty(B, L_out, device=dev, dtype=torch.float32) if target is not None else None
    ws, ws_bytes = _WS.get(lib.pd_loudness_workspace_size(h, B, L, nb), dev)
    _lib.check(lib.pd_loudness_forward(h, _lib.fptr(y), _lib.iptr(ln), _lib.iptr(bounds), _lib.iptr(cnt), nb,
                                       float(target if target is not None else 0.0), _lib.C.c_void_p(loud.data_ptr()),
                                       _lib.fptr(peak), _lib.fptr(out), B, L, int(L_out or 0), ws, ws_bytes,
                                       _lib.stream_ptr(dev)))
    return loud, peak, out


def _pick_device(device, tensors):
    if device is None:
        device = next((t.device for t in tensors if t.is_cuda), None)
    if device is None:
        if not torch.cuda.is_available():
            raise _lib.HipError("the analysis runs on the GPU only (none is visible; there is no CPU fallback)")
        device = "cuda"
    return torch.device(device)


def _to_device(t, device):
    return t.to(_pick_device(device, [t])).float().contiguous()


@torch.no_grad()
def integrated_loudness(wav, rate, lens=None, device=None):
    """``pyloudnorm.Meter(rate).integrated_loudness(wav)`` for mono ``wav`` [L] or a batch [B, L] (``lens``:
    samples per row, host values).  A numpy input gives numpy float64 (a scalar for [L]), a tensor gives a
    float64 tensor on the GPU.  -inf when no block passes the gates; ValueError below one 400 ms block."""
    t, host, single = _as_batch(wav, lens, device)
    _check_lengths(host, rate)
    loud, _, _ = _measure(_to_device(t, device), host, rate)
    if not torch.is_tensor(wav):
        loud = loud.cpu().numpy()
        return float(loud[0]) if single else loud
    return loud[0] if single else loud


@torch.no_grad()
def normalize_loudness(wav, rate, target, lens=None, device=None):
    """process_utterance :118-122: measure, ``pyloudnorm.normalize.loudness(wav, loudness, target)`` in float32,
    then divide by the peak when it exceeds 1.  Same shape as ``wav`` (samples past a row's ``lens`` are 0);
    numpy in, numpy out."""
    t, host, single = _as_batch(wav, lens, device)
    _check_lengths(host, rate)
    _, _, out = _measure(_to_device(t, device), host, rate, float(target), t.shape[1])
    out = out[0] if single else out
    return out if torch.is_tensor(wav) else out.cpu().numpy()


# ---------------------------------------------------------------- process_utterance
class CenteredZeroMel(MelFrontEnd):
    """librosa.stft(n_fft, hop, win, "hann", center=True, pad_mode="constant") -> |X| -> Slaney mel, plain
    (``log10=False``, vocoder='fastdiff') or log10(max(eps, mel)) ('pwg'), on pd_mel_create_centered_zero."""

    def __init__(self, sample_rate, fft_size, hop_size, win_length, num_mels, fmin, fmax, eps, log10):
        basis = mel_filterbank(sample_rate, fft_size, num_mels, fmin, fmax)
        mode = _lib.PD_MEL_OUT_LOG10 if log10 else _lib.PD_MEL_OUT_LINEAR
        self._setup("process_utterance", "pd_mel_create_centered_zero", basis, fft_size, win_length, hop_size, eps,
                    create_extra=(mode,))

    def _min_samples(self, keyshift, speed):
        return 1, "zero padding needs"


_FRONTS = {}


def _front(*key):
    f = _FRONTS.get(key)
    if f is None:
        if len(_FRONTS) >= 8:
            _FRONTS.pop(next(iter(_FRONTS))).close()
        f = _FRONTS[key] = CenteredZeroMel(*key)
    return f


@torch.no_grad()
def process_utterance(wav_path, fft_size=1024, hop_size=256, win_length=1024, window="hann", num_mels=80, fmin=80,
                      fmax=7600, eps=1e-6, sample_rate=22050, loud_norm=False, min_level_db=-100, return_linear=False,
                      trim_long_sil=False, vocoder="pwg", to_numpy=True, device=None, lens=None):
    """utils/data_gen_utils.py:95-149.  ``wav_path``: the path of a WAV at ``sample_rate`` (there is no resampler
    in this call), a mono float array / tensor [L], or a list of such clips (a ragged batch: one launch chain,
    every clip's result equal to that clip alone), or the padded batch itself as an array / tensor [B, L] with
    ``lens`` (what a row holds past its length is never read).  Returns (wav [T hop], mel [num_mels, T][, spc
    [fft_size // 2 + 1, T]]) in the reference's shapes, T = 1 + L // hop_size -- lists of them for a list of
    clips; numpy arrays, or device tensors with ``to_numpy=False``.  The mel is linear unless ``vocoder == 'pwg'``
    (log10(max(eps, mel)))."""
    if trim_long_sil:
        raise NotImplementedError("trim_long_sil=True is not offered: the reference trims with webrtcvad "
                                  "(utils/data_gen_utils.py:29-92), which this library does not restate")
    if window != "hann":
        raise NotImplementedError(f"window {window!r}: only 'hann' is offered")
    many = isinstance(wav_path, (list, tuple))
    if not many and not isinstance(wav_path, (str, os.PathLike)) and np.ndim(wav_path) == 2:
        t, lens, _ = _as_batch(wav_path, lens, device)
        if min(lens) < 1:
            raise ValueError("every row must hold at least one sample")
        wav_path, many = [t[i, :n] for i, n in enumerate(lens)], True
    elif lens is not None:
        raise ValueError("lens goes with a padded batch [B, L]")
    clips = []
    for c in (wav_path if many else [wav_path]):
        if isinstance(c, (str, os.PathLike)):
            c = read_wav(c, sample_rate)
        c = c.detach() if torch.is_tensor(c) else torch.from_numpy(np.ascontiguousarray(np.asarray(c, np.float32)))
        if c.dim() != 1 or c.numel() < 1:
            raise ValueError(f"a clip must be a non-empty mono signal [L], got {tuple(c.shape)}")
        clips.append(c.float())
    lens = [int(c.numel()) for c in clips]
    if loud_norm:
        _check_lengths(lens, sample_rate)
    fmin = 0 if fmin == -1 else fmin
    fmax = sample_rate / 2 if fmax == -1 else fmax
    dev = _pick_device(device, clips)
    B, L = len(clips), max(lens)
    if B == 1:
        y = clips[0].to(dev)[None].contiguous()
    else:
        y = torch.zeros(B, L, device=dev, dtype=torch.float32)
        for i, c in enumerate(clips):
            y[i, :lens[i]] = c.to(dev)
    L_out = (1 + L // hop_size) * hop_size       # librosa_pad_lr, then the trim to mel.shape[1] * hop_size
    if loud_norm:
        _, _, wav = _measure(y, lens, sample_rate, TARGET_LUFS, L_out)
    else:
        wav = torch.empty(B, L_out, device=dev, dtype=torch.float32)
        ln = None if B == 1 else _lib._device_rows(lens, B, dev, "lens", 1, L)
        _lib.check(_lib.lib().pd_loudness_pad(_lib.fptr(y), _lib.iptr(ln), _lib.fptr(wav), B, L, L_out,
                                              _lib.stream_ptr(dev)))
    front = _front(int(sample_rate), int(fft_size), int(hop_size), int(win_length), int(num_mels), float(fmin),
                   float(fmax), float(eps), vocoder == "pwg")
    # the padded buffer holds one hop more than the clip: its last frame is dropped below
    res = front._mel_time_major(wav, 0, 1, lens=lens, return_spec=return_linear)
    mel, spc = res if return_linear else (res, None)
    if return_linear:
        _lib.check(_lib.lib().pd_mel_normalize_spec(_lib.fptr(spc), float(min_level_db), _lib.fptr(spc), spc.numel(),
                                                    _lib.stream_ptr(dev)))
    if to_numpy:
        wav, mel = wav.cpu().numpy(), mel.cpu().numpy()
        spc = spc.cpu().numpy() if return_linear else None
    out = []
    for i, n in enumerate(lens):
        T = 1 + n // hop_size
        row = (wav[i, :T * hop_size], mel[i, :T].T)
        out.append(row + (spc[i, :T].T,) if return_linear else row)
    if many:
        return tuple(list(col) for col in zip(*out))
    return out[0]
