"""Variance curves and k-th harmonic isolation on the GPU: the reference's component/binarizer/binarizer_utils.py
``get_energy`` / ``get_voicing`` / ``get_breath`` / ``get_kth_harmonic`` / ``get_tension`` (:115-213) and
modules/commons/common_layers.py ``SinusoidalSmoothingConv1d`` (:974-988) on pd_curves (include/prodiff_hip.h,
"variance curves").  ``librosa.feature.rms`` and ``librosa.amplitude_to_db`` of librosa 0.8.0 are restated in the
kernels, so no librosa is needed.  Inference only, fp32 only.

Every function takes the reference's numpy arrays and returns numpy, or takes CUDA tensors (a waveform [L] or
[B, L], f0 [T] or [B, T]) and returns tensors without touching the host.

Ragged batches: clips of different lengths go through one call as a list of clips with a list of f0 curves, or as
padded tensors with ``lens`` (samples per row) and ``f0_lens`` (f0 frames per row), B host ints each; ``mel_len``
may then be an int or B ints.  Every row's result equals, bit for bit, that clip's own call.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib

MIN_KERNEL, MAX_KERNEL = 3, 257
_PAD = {"reflect": 0, "constant": 1}
_ENERGY = {"amplitude": 0, "db": 1}
_TENSION = {"ratio": 0, "db": 1, "logit": 2}


def smoothing_taps(kernel_size):
    """common_layers.py:984-987: sin(linspace(0, 1, k) pi) in float32 over its float32 sum."""
    if int(kernel_size) != kernel_size or kernel_size < MIN_KERNEL:
        raise ValueError(f"kernel_size must be an integer >= {MIN_KERNEL} (the reference's taps are 0/0 or "
                         f"meaningless below), got {kernel_size}")
    if kernel_size > MAX_KERNEL:
        raise _lib.HipError(f"kernel_size must lie in [{MIN_KERNEL}, {MAX_KERNEL}], got {kernel_size}")
    k = torch.sin(torch.from_numpy(np.linspace(0, 1, int(kernel_size)).astype(np.float32) * np.pi))
    k /= k.sum()
    return k


def same_padding(kernel_size):
    """(left, right) frames that Conv1d(padding='same', padding_mode='replicate') replicates."""
    total = int(kernel_size) - 1
    return total // 2, total - total // 2


def num_frames(n_samples, hop_size):
    """Frames of the centred STFT and of librosa.feature.rms for a signal of n_samples."""
    return int(n_samples) // int(hop_size) + 1


def kept_bins(center, win_size, half_width=3.5):
    """(first kept bin, count) per frame from the float32 centres, by the f0 kernel's arithmetic: bin i is kept
    iff center >= 1 and max(center - hw, 0) <= i < min(center + hw, n_bins), so first = ceil(start) and the count
    is ceil(end) - first, at most 8."""
    c = np.asarray(center, np.float32)
    n_bins, hw = np.float32(win_size // 2 + 1), np.float32(half_width)
    with np.errstate(invalid="ignore"):
        ok = (c >= 1) & (c <= np.float32(3.0e38))
        cc = np.where(ok, c, np.float32(1))
        start = np.minimum(np.maximum(cc - hw, np.float32(0)), n_bins)
        end = np.maximum(np.minimum(cc + hw, n_bins), np.float32(0))
    first = np.ceil(start).astype(np.int64)
    count = np.clip(np.ceil(end).astype(np.int64) - first, 0, 8)
    return np.where(ok, first, 0), np.where(ok, count, 0)


def curve_rows(lens, mel_len, f0_lens, L, T_f0, win_size, hop_size):
    """The (L_b, mel_len_b, T_f0_b) rows of a ragged call from host values, checked as the equal-length calls
    check their own: ``lens`` B ints or None (every row L samples), ``mel_len`` an int, B ints or None (each
    row's frame count), ``f0_lens`` B ints or None (every row T_f0 frames; T_f0 = 0: the call takes no f0)."""
    if any(torch.is_tensor(v) and v.is_cuda for v in (lens, mel_len, f0_lens)):
        raise _lib.HipError("variance curves: `lens`, `f0_lens` and `mel_len` must be host integers (the per-row "
                            "sizes are worked out on the host)")
    host = lambda v: [int(x) for x in (v.tolist() if torch.is_tensor(v) else v)]   # noqa: E731
    B = len(host(lens)) if lens is not None else (len(host(f0_lens)) if f0_lens is not None else len(host(mel_len)))
    ls = [int(L)] * B if lens is None else host(lens)
    fs = [int(T_f0)] * B if f0_lens is None else host(f0_lens)
    if mel_len is None:
        ms = [num_frames(n, hop_size) for n in ls]
    else:
        ms = [int(mel_len)] * B if np.ndim(mel_len) == 0 else host(mel_len)
    if not len(ls) == len(ms) == len(fs) == B:
        raise _lib.HipError(f"lens, mel_len and f0_lens hold {len(ls)}, {len(ms)} and {len(fs)} values for one batch")
    for b, (n, m, f) in enumerate(zip(ls, ms, fs)):
        if not win_size // 2 < n <= L:
            raise _lib.HipError(f"row {b}: n_samples must exceed win_size / 2 = {win_size // 2} (reflect padding) and "
                                f"fit the row stride {L}, got {n}")
        if m < 1:
            raise _lib.HipError(f"row {b}: mel_len must be positive, got {m}")
        if T_f0 and not 1 <= f <= T_f0:
            raise _lib.HipError(f"row {b}: f0 must hold between 1 and {T_f0} frames, got {f}")
    return list(zip(ls, ms, fs))


def check_dims(win_size, hop_size, half_width=3.5):
    """The dimensions pd_curves_create takes; raises HipError naming the first one outside them."""
    if win_size % 64 != 0 or not 64 <= win_size <= 4096:
        raise _lib.HipError(f"win_size must be a multiple of 64 in [64, 4096], got {win_size}")
    if hop_size < 1 or win_size % hop_size != 0 or not 2 <= win_size // hop_size <= 16:
        raise _lib.HipError(f"hop_size must divide win_size with win_size / hop_size in [2, 16], got {hop_size}")
    if not 0 < half_width <= 3.5:
        raise _lib.HipError(f"half_width must lie in (0, 3.5], got {half_width}")


class SinusoidalSmoothingConv1d:
    """common_layers.py:974-988 (inference only): ``weight`` [1, 1, k] holds the reference's taps bit for bit.
    Called on a CUDA tensor [..., T] it smooths every row natively (replicate padding, 'same' length); handed
    to the functions below as ``smooth_func`` its taps go into their kernels."""

    def __init__(self, kernel_size):
        self.kernel_size = int(kernel_size)
        self.weight = smoothing_taps(kernel_size)[None, None]
        self._dev = {}

    def taps(self, device):
        device = torch.device(device)
        t = self._dev.get(str(device))
        if t is None:
            t = self._dev[str(device)] = self.weight.reshape(-1).to(device).contiguous()
        return t

    @torch.no_grad()
    def __call__(self, x):
        if not x.is_cuda:
            raise _lib.HipError("SinusoidalSmoothingConv1d runs on the GPU (got a CPU tensor; there is no CPU fallback)")
        rows = x.float().contiguous().reshape(-1, x.shape[-1])
        out = torch.empty_like(rows)
        _lib.check(_lib.lib().pd_curves_smooth(_lib.fptr(rows), _lib.fptr(self.taps(x.device)), self.kernel_size,
                                               _lib.fptr(out), rows.shape[0], rows.shape[1], _lib.stream_ptr(x.device)))
        return out.reshape(x.shape)

    forward = __call__


class _Core:
    """One (samplerate, win_size, hop_size, half_width): its native handles (one per device) and workspace."""

    def __init__(self, samplerate, win_size, hop_size, half_width=3.5):
        self.samplerate, self.win_size, self.hop_size = int(samplerate), int(win_size), int(hop_size)
        self.half_width = float(half_width)
        if self.samplerate < 1:
            raise _lib.HipError(f"samplerate must be positive, got {samplerate}")
        check_dims(self.win_size, self.hop_size, self.half_width)
        self._cache = _lib.HandleCache("variance curves", "pd_curves_create", "pd_curves_destroy")
        self.handles = self._cache.handles
        self._ws = _lib.Workspace()

    def handle(self, device):
        dims = _lib.pd_curves_dims(self.samplerate, self.win_size, self.hop_size, self.half_width)
        return self._cache.get(device, (), lambda device: (dims, []))

    def close(self):
        self._cache.close()

    def _rows(self, wav, name="waveform"):
        if wav.dim() not in (1, 2):
            raise ValueError(f"expected a {name} [L] or [B, L], got {tuple(wav.shape)}")
        x = wav.float().contiguous()
        x = x[None] if x.dim() == 1 else x
        if x.shape[1] <= self.win_size // 2:
            raise _lib.HipError(f"n_samples must exceed win_size / 2 = {self.win_size // 2} (reflect padding), "
                                f"got {x.shape[1]}")
        return x

    def _f0(self, f0, B):
        f = f0.float().contiguous()
        f = f[None] if f.dim() == 1 else f
        if f.dim() != 2 or f.shape[0] != B:
            raise ValueError(f"expected f0 [T] or [{B}, T], got {tuple(f0.shape)}")
        if f.shape[1] < 1:
            raise _lib.HipError("f0 must hold at least one frame, got 0")
        return f

    def _workspace(self, h, B, L, T_f0, dev):
        return self._ws.get(_lib.lib().pd_curves_workspace_size(h, B, L, T_f0), dev)

    def _ragged(self, B, L, T_f0, lens, mel_len, f0_lens, dev):
        """-> (the host triples, their cached device int32 copy [B, 3]) of a ragged call."""
        rows = curve_rows(lens, mel_len, f0_lens, L, T_f0, self.win_size, self.hop_size)
        if len(rows) != B:
            raise _lib.HipError(f"the per-row sizes hold {len(rows)} values for a batch of {B}")
        return rows, _lib._device_rows([v for r in rows for v in r], 3 * B, dev, "curve_rows", 0, 2 ** 31 - 1)

    @torch.no_grad()
    def kth_harmonic(self, k, wav, f0, resid=False, lens=None, f0_lens=None):
        """``lens`` / ``f0_lens`` (B host ints): a ragged batch (pd_curves_kth_harmonic_ragged) -- row b is its
        first lens[b] samples with its first f0_lens[b] f0 frames; the outputs are 0 past lens[b]."""
        x = self._rows(wav, "harmonic part")
        B, L = x.shape
        f = self._f0(f0, B)
        if k < 0:
            raise _lib.HipError(f"k must not be negative, got {k}")
        h = self.handle(x.device)
        rd = None
        if lens is not None or f0_lens is not None:
            rd = self._ragged(B, L, f.shape[1], lens, 1, f0_lens, x.device)[1]
        y = torch.empty_like(x)
        r = torch.empty_like(x) if resid else None
        ws, wsb = self._workspace(h, B, L, f.shape[1], x.device)
        if rd is not None:
            _lib.check(_lib.lib().pd_curves_kth_harmonic_ragged(h, _lib.fptr(x), _lib.fptr(f), int(k), _lib.fptr(y),
                                                                _lib.fptr(r), _lib.iptr(rd), B, L, f.shape[1], ws, wsb,
                                                                _lib.stream_ptr(x.device)))
            return (y, r) if resid else y
        _lib.check(_lib.lib().pd_curves_kth_harmonic(h, _lib.fptr(x), _lib.fptr(f), int(k), _lib.fptr(y), _lib.fptr(r),
                                                     B, L, f.shape[1], ws, wsb, _lib.stream_ptr(x.device)))
        y = y[0] if wav.dim() == 1 else y
        return (y, r[0] if wav.dim() == 1 else r) if resid else y

    @torch.no_grad()
    def energy(self, wav, mel_len, domain="db", smooth=None, norm=False, db_min=-96.0, db_max=-12.0, pad_mode="reflect",
               lens=None):
        """``lens`` (B host ints) or a ``mel_len`` of B ints: a ragged batch (pd_curves_energy_ragged) -> out
        [B, max mel_len], row b's first mel_len[b] frames its own curve, 0 past them."""
        if domain not in _ENERGY:
            raise ValueError(f"Unknown domain: {domain}")
        x = self._rows(wav)
        B, L = x.shape
        h = self.handle(x.device)
        taps, ks = (smooth.taps(x.device), smooth.kernel_size) if smooth is not None else (None, 0)
        ws, wsb = self._workspace(h, B, L, 0, x.device)
        if lens is not None or np.ndim(mel_len) != 0:
            rows, rd = self._ragged(B, L, 0, lens, mel_len, None, x.device)
            width = max(r[1] for r in rows)
            out = torch.empty(B, width, device=x.device, dtype=torch.float32)
            _lib.check(_lib.lib().pd_curves_energy_ragged(h, _lib.fptr(x), _pad_mode(pad_mode), _ENERGY[domain], width,
                                                          _lib.fptr(taps), ks, int(bool(norm)), float(db_min),
                                                          float(db_max), _lib.fptr(out), _lib.iptr(rd), B, L, ws, wsb,
                                                          _lib.stream_ptr(x.device)))
            return out
        out = torch.empty(B, int(mel_len), device=x.device, dtype=torch.float32)
        _lib.check(_lib.lib().pd_curves_energy(h, _lib.fptr(x), _pad_mode(pad_mode), _ENERGY[domain], int(mel_len),
                                               _lib.fptr(taps), ks, int(bool(norm)), float(db_min), float(db_max),
                                               _lib.fptr(out), B, L, ws, wsb, _lib.stream_ptr(x.device)))
        return out[0] if wav.dim() == 1 else out

    @torch.no_grad()
    def forward(self, sp, ap, f0, mel_len, smooth=None, tension_domain="logit", norm=True, db_min=-96.0, db_max=-12.0,
                pad_mode="reflect", want_curves=True, return_base=False, lens=None, f0_lens=None):
        """The fused call -> (voicing, breath, tension, base); voicing and breath are None without
        ``want_curves`` (get_tension alone), base is None without ``return_base``.  ``lens`` / ``f0_lens`` (B host
        ints each) or a ``mel_len`` of B ints: a ragged batch (pd_curves_forward_ragged) -> curves [B, max mel_len]
        and base [B, L], every row its own call's result, 0 past its mel_len and its samples."""
        if tension_domain not in _TENSION:
            raise ValueError(f"Unknown domain: {tension_domain}")
        x = self._rows(sp, "harmonic part")
        B, L = x.shape
        f = self._f0(f0, B)
        a = None
        if want_curves:
            a = self._rows(ap, "aperiodic part")
            if a.shape != x.shape:
                raise ValueError(f"the harmonic and aperiodic parts differ in shape: {tuple(x.shape)}, {tuple(a.shape)}")
        h = self.handle(x.device)
        rd, width = None, mel_len
        if lens is not None or f0_lens is not None or np.ndim(mel_len) != 0:
            rows, rd = self._ragged(B, L, f.shape[1], lens, mel_len, f0_lens, x.device)
            width = max(r[1] for r in rows)
        new = lambda: torch.empty(B, int(width), device=x.device, dtype=torch.float32)   # noqa: E731
        tension = new()
        voicing, breath = (new(), new()) if want_curves else (None, None)
        base = torch.empty_like(x) if return_base else None
        taps, ks = (smooth.taps(x.device), smooth.kernel_size) if smooth is not None else (None, 0)
        ws, wsb = self._workspace(h, B, L, f.shape[1], x.device)
        if rd is not None:
            _lib.check(_lib.lib().pd_curves_forward_ragged(h, _lib.fptr(x), _lib.fptr(a), _lib.fptr(f), _pad_mode(pad_mode),
                                                           _TENSION[tension_domain], int(width), _lib.fptr(taps), ks,
                                                           int(bool(norm)), float(db_min), float(db_max),
                                                           _lib.fptr(voicing), _lib.fptr(breath), _lib.fptr(tension),
                                                           _lib.fptr(base), _lib.iptr(rd), B, L, f.shape[1], ws, wsb,
                                                           _lib.stream_ptr(x.device)))
            return voicing, breath, tension, base
        _lib.check(_lib.lib().pd_curves_forward(h, _lib.fptr(x), _lib.fptr(a), _lib.fptr(f), _pad_mode(pad_mode),
                                                _TENSION[tension_domain], int(mel_len), _lib.fptr(taps), ks,
                                                int(bool(norm)), float(db_min), float(db_max), _lib.fptr(voicing),
                                                _lib.fptr(breath), _lib.fptr(tension), _lib.fptr(base), B, L,
                                                f.shape[1], ws, wsb, _lib.stream_ptr(x.device)))
        if sp.dim() == 1:
            voicing, breath, tension, base = [None if t is None else t[0] for t in (voicing, breath, tension, base)]
        return voicing, breath, tension, base


def _pad_mode(pad_mode):
    if pad_mode not in _PAD:
        raise ValueError(f"pad_mode must be 'reflect' or 'constant', got {pad_mode!r}")
    return _PAD[pad_mode]


_CORES = {}


def _core(samplerate, win_size, hop_size, half_width=3.5):
    """The module-level handles behind the reference's free functions (a small cache, oldest out first)."""
    key = (int(samplerate), int(win_size), int(hop_size), float(half_width))
    c = _CORES.get(key)
    if c is None:
        if len(_CORES) >= 8:
            _CORES.pop(next(iter(_CORES))).close()
        c = _CORES[key] = _Core(*key)
    return c


def close_all():
    """Destroy the handles behind the free functions (every device byte goes back)."""
    for c in _CORES.values():
        c.close()
    _CORES.clear()


def _front(device, *arrays):
    """numpy inputs -> (True, CUDA tensors on ``device``); CUDA tensors -> (False, themselves)."""
    if all(torch.is_tensor(a) for a in arrays):
        return False, arrays
    return True, [torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).to(device) for a in arrays]


def _back(as_numpy, t):
    return t.cpu().numpy() if as_numpy else t


def _is_ragged(x, *lens):
    return isinstance(x, (list, tuple)) or any(v is not None for v in lens)


def _stack(rows, lens, device):
    """A ragged batch of clips or f0 curves (``rmvpe.stack_waveforms``: a list of 1-D arrays, or a padded [B, n]
    with ``lens``) -> (as_numpy, float32 [B, n_max] on the device, B host counts)."""
    from .rmvpe import stack_waveforms
    first = rows[0] if isinstance(rows, (list, tuple)) and len(rows) else rows
    t, ns = stack_waveforms(rows, lens, device)
    return not torch.is_tensor(first), t, ns


def _cut(as_numpy, t, ns):
    """The rows of a padded result, each cut to its own length."""
    return None if t is None else [_back(as_numpy, t[b, :n]) for b, n in enumerate(ns)]


def _apply(smooth_func, curve):
    """A foreign ``smooth_func`` on the unsmoothed curve [T] or [B, T], as the reference calls it: rows one by one."""
    if curve.dim() == 1:
        return smooth_func(curve[None])[0]
    return torch.stack([smooth_func(r[None])[0] for r in curve])


def _norm(x, db_min, db_max):
    return (torch.clamp(x, db_min, db_max) - db_min) / (db_max - db_min)


def get_energy(waveform, mel_len, hop_size, win_size, domain="db", pad_mode="reflect", device="cuda"):
    """binarizer_utils.py:115-126.  The sample rate does not enter (any handle of this window and hop serves)."""
    if domain not in _ENERGY:
        raise ValueError(f"Unknown domain: {domain}")
    as_np, (wav,) = _front(device, waveform)
    return _back(as_np, _core(1, win_size, hop_size).energy(wav, mel_len, domain, pad_mode=pad_mode))


def _db_curve(wav, mel_len, hop_size, win_size, smooth_func, norm, db_min, db_max, device, pad_mode, lens=None):
    core = _core(1, win_size, hop_size)
    if _is_ragged(wav, lens) or np.ndim(mel_len) != 0:
        # a ragged batch -> a list of curves; a foreign smooth_func sees each row's unsmoothed curve cut to its mel_len
        as_np, x, ns = _stack(wav, lens, device)
        ms = [r[1] for r in curve_rows(ns, mel_len, None, x.shape[1], 0, win_size, hop_size)]
        if isinstance(smooth_func, SinusoidalSmoothingConv1d):
            return _cut(as_np, core.energy(x, ms, "db", smooth_func, norm, db_min, db_max, pad_mode, lens=ns), ms)
        raw = core.energy(x, ms, "db", pad_mode=pad_mode, lens=ns)
        out = [smooth_func(raw[b, :m][None])[0] for b, m in enumerate(ms)]
        return [_back(as_np, (_norm(o, db_min, db_max) if norm else o).detach()) for o in out]
    as_np, (x,) = _front(device, wav)
    if isinstance(smooth_func, SinusoidalSmoothingConv1d):
        out = core.energy(x, mel_len, "db", smooth_func, norm, db_min, db_max, pad_mode)
    else:
        out = _apply(smooth_func, core.energy(x, mel_len, "db", pad_mode=pad_mode))
        out = _norm(out, db_min, db_max) if norm else out
    return _back(as_np, out.detach())


def get_voicing(sp, mel_len, hop_size, win_size, smooth_func, norm=True, db_min=-96.0, db_max=-12.0, device="cuda",
                pad_mode="reflect", lens=None):
    """binarizer_utils.py:128-134.  A list of clips, or a padded [B, L] with ``lens``, gives a list of curves."""
    return _db_curve(sp, mel_len, hop_size, win_size, smooth_func, norm, db_min, db_max, device, pad_mode, lens)


def get_breath(ap, mel_len, hop_size, win_size, smooth_func, norm=True, db_min=-96.0, db_max=-12.0, device="cuda",
               pad_mode="reflect", lens=None):
    """binarizer_utils.py:136-142.  A list of clips, or a padded [B, L] with ``lens``, gives a list of curves."""
    return _db_curve(ap, mel_len, hop_size, win_size, smooth_func, norm, db_min, db_max, device, pad_mode, lens)


def get_kth_harmonic(k, harmonic_part, f0, hop_size, win_size, samplerate, half_width=3.5, device="cuda"):
    """binarizer_utils.py:144-194."""
    as_np, (wav, f) = _front(device, harmonic_part, f0)
    return _back(as_np, _core(samplerate, win_size, hop_size, half_width).kth_harmonic(k, wav, f))


def get_tension(sp, mel_len, f0, hop_size, win_size, samplerate, smooth_func, half_width=3.5, domain="logit",
                device="cuda", pad_mode="reflect"):
    """binarizer_utils.py:196-213.  A ``domain`` the reference does not know raises (the reference would smooth the
    unclipped ratio)."""
    as_np, (wav, f) = _front(device, sp, f0)
    core = _core(samplerate, win_size, hop_size, half_width)
    native = isinstance(smooth_func, SinusoidalSmoothingConv1d)
    t = core.forward(wav, None, f, mel_len, smooth_func if native else None, domain, pad_mode=pad_mode,
                     want_curves=False)[2]
    if not native:
        t = _apply(smooth_func, t)
    return _back(as_np, t.detach())


class VarianceCurves:
    """The three curves of one binarizer item in a single native call.  ``smooth_width`` seconds give the
    reference's kernel_size = round(smooth_width / (hop_size / samplerate)) (component/binarizer/svs.py:140-146)."""

    def __init__(self, samplerate, win_size, hop_size, smooth_width=0.12, half_width=3.5, tension_domain="logit",
                 norm=True, db_min=-96.0, db_max=-12.0, pad_mode="reflect"):
        if tension_domain not in _TENSION:
            raise ValueError(f"Unknown domain: {tension_domain}")
        _pad_mode(pad_mode)
        self.core = _Core(samplerate, win_size, hop_size, half_width)
        self.smooth = SinusoidalSmoothingConv1d(round(smooth_width / (hop_size / samplerate)))
        self.tension_domain, self.norm, self.db_min, self.db_max = tension_domain, norm, db_min, db_max
        self.pad_mode = pad_mode

    def close(self):
        self.core.close()

    def __call__(self, sp, ap, f0, mel_len, return_base=False, device="cuda", lens=None, f0_lens=None):
        """A ragged batch -- lists of clips with a list of f0 curves, or padded tensors with ``lens`` and
        ``f0_lens``; ``mel_len`` an int, B ints or None (each row's frame count) -- gives lists of per-row curves
        cut to each row's mel_len (the base harmonic to its samples)."""
        if _is_ragged(sp, lens, f0_lens) or np.ndim(mel_len) != 0:
            as_np, s, ns = _stack(sp, lens, device)
            _, a, na = _stack(ap, lens, device)
            _, f, nf = _stack(f0, f0_lens, device)
            if na != ns:
                raise ValueError(f"the harmonic and aperiodic parts differ in length: {ns}, {na}")
            ms = [r[1] for r in curve_rows(ns, mel_len, nf, s.shape[1], f.shape[1], self.core.win_size,
                                           self.core.hop_size)]
            v, b, t, base = self.core.forward(s, a, f, ms, self.smooth, self.tension_domain, self.norm, self.db_min,
                                              self.db_max, self.pad_mode, True, return_base, lens=ns, f0_lens=nf)
            out = dict(voicing=_cut(as_np, v, ms), breath=_cut(as_np, b, ms), tension=_cut(as_np, t, ms))
            if return_base:
                out["base_harmonic"] = _cut(as_np, base, ns)
            return out
        as_np, (s, a, f) = _front(device, sp, ap, f0)
        v, b, t, base = self.core.forward(s, a, f, mel_len, self.smooth, self.tension_domain, self.norm, self.db_min,
                                          self.db_max, self.pad_mode, True, return_base)
        out = dict(voicing=_back(as_np, v), breath=_back(as_np, b), tension=_back(as_np, t))
        if return_base:
            out["base_harmonic"] = _back(as_np, base)
        return out

    def extract_variance_curves(self, waveform, f0, sep_model, mel_len=None, return_base=False, lens=None,
                                f0_lens=None):
        """A mono waveform [L] or [B, L] (numpy or CUDA tensor) and its f0 -> the curves, through
        ``sep_model.separate`` (a mono CascadedNet) on the current stream.  mel_len: the frame count by default.
        A ragged batch (a list of clips with a list of f0, or padded tensors with ``lens`` and ``f0_lens``) runs
        one ragged ``separate`` and one ragged curves call and gives lists of per-row curves.  The separation runs
        in ``sep_model``'s compute dtype (``CascadedNet.set_compute_dtype``); the curves themselves stay fp32."""
        dev = next(sep_model.parameters()).device
        if _is_ragged(waveform, lens, f0_lens):
            as_np, wav, ns = _stack(waveform, lens, dev)
            _, f, nf = _stack(f0, f0_lens, dev)
            sp, ap = _separate_mono(sep_model, wav, ns)
            out = self(sp, ap, f, mel_len, return_base, dev, lens=ns, f0_lens=nf)
            return {k: [_back(as_np, r) for r in v] for k, v in out.items()}
        as_np, (wav, f) = _front(dev, waveform, f0)
        sp, ap = _separate_mono(sep_model, wav)
        mel_len = num_frames(wav.shape[-1], self.core.hop_size) if mel_len is None else mel_len
        out = self(sp, ap, f, mel_len, return_base)
        return {k: _back(as_np, v) for k, v in out.items()}


def _separate_mono(sep_model, wav, lens=None):
    """extract_harmonic_aperiodic (binarizer_utils.py:99-113) on device tensors [L] or [B, L]; ``lens``: a ragged
    batch (``CascadedNet.separate``), the parts are then meaningful below each row's own length."""
    x = wav[None] if wav.dim() == 1 else wav
    x = x[:, None].float()
    if sep_model.is_mono:
        y, ap = sep_model.separate(x, lens)
        sp, ap = y[:, 0], ap[:, 0]
    else:
        sp = sep_model.separate(x.repeat(1, 2, 1), lens)[0].mean(dim=1)
        ap = x[:, 0] - sp
    return (sp[0], ap[0]) if wav.dim() == 1 else (sp, ap)


def isolate_parts(wav, f0, sep_model, hop_size, win_size, samplerate, base_harmonic=False, lens=None, f0_lens=None):
    """handler/infer/handler.py:349-358: a vocoder output -> (sp, ap), or with ``base_harmonic``
    (sp - base, ap, base), the subtraction from the synthesis kernel's epilogue.  A ragged batch (a list of
    segments with a list of f0, or padded tensors with ``lens`` and ``f0_lens``) gives lists, each row cut to its
    own samples, from one ragged ``separate`` and one ragged ``kth_harmonic`` call.  The separation runs in
    ``sep_model``'s compute dtype (``CascadedNet.set_compute_dtype``)."""
    dev = next(sep_model.parameters()).device
    if _is_ragged(wav, lens, f0_lens):
        as_np, x, ns = _stack(wav, lens, dev)
        sp, ap = _separate_mono(sep_model, x, ns)
        if not base_harmonic:
            return _cut(as_np, sp, ns), _cut(as_np, ap, ns)
        _, f, nf = _stack(f0, f0_lens, dev)
        base, rest = _core(samplerate, win_size, hop_size).kth_harmonic(0, sp, f, resid=True, lens=ns, f0_lens=nf)
        return _cut(as_np, rest, ns), _cut(as_np, ap, ns), _cut(as_np, base, ns)
    as_np, (x, f) = _front(dev, wav, f0)
    sp, ap = _separate_mono(sep_model, x)
    if not base_harmonic:
        return _back(as_np, sp), _back(as_np, ap)
    base, rest = _core(samplerate, win_size, hop_size).kth_harmonic(0, sp, f, resid=True)
    return _back(as_np, rest), _back(as_np, ap), _back(as_np, base)
