"""RMVPE pitch extraction on the GPU: the reference's modules/rmvpe (``E2E0``, ``MelSpectrogram``,
``to_local_average_f0``) and component/pe/rmvpe.py (``RMVPE``) on pd_rmvpe, the centred pd_mel and pd_resample
(include/prodiff_hip.h, "pitch extraction").  No librosa, no torchaudio.  fp32 is the default;
``E2E0.set_compute_dtype("bf16")`` runs the 3x3 convs and the recurrent product on the bf16 MFMA
(pd_rmvpe_set_option), all else staying fp32.
"""
from __future__ import annotations

import numpy as np
import torch
from torch import nn

from . import _lib, synth
from .mel import MelFrontEnd, derived_sizes, mel_filterbank
from .resample import Resample

SAMPLE_RATE, N_CLASS, N_MELS = 16000, synth.RMVPE_N_CLASS, synth.RMVPE_N_MELS      # modules/rmvpe/constants.py
MEL_FMIN, MEL_FMAX, WINDOW_LENGTH = 30, 8000, 1024
CONST = 1997.3794084376191

PITCH_EXTRACTORS = {}


def register_pe(cls):
    """component/pe/base.py: the registry ``get_pitch_extractor_cls`` reads."""
    PITCH_EXTRACTORS[cls.__name__.lower()] = cls
    PITCH_EXTRACTORS[cls.__name__] = cls
    return cls


def get_pitch_extractor_cls(name):
    if name.lower() not in PITCH_EXTRACTORS:
        raise ValueError(f"Pitch extractor {name.lower()} not found in PITCH_EXTRACTORS")
    return PITCH_EXTRACTORS[name.lower()]


# ---------------------------------------------------------------- network
def _attach(root, key, tensor, buffer):
    """Register ``tensor`` under the dotted state-dict key, creating the modules on the way."""
    *path, leaf = key.split(".")
    mod = root
    for name in path:
        if name not in mod._modules:
            mod.add_module(name, nn.Module())
        mod = mod._modules[name]
    if buffer:
        mod.register_buffer(leaf, tensor)
    else:
        mod.register_parameter(leaf, nn.Parameter(tensor, requires_grad=False))


class E2E0(nn.Module):
    """modules/rmvpe/model.py:8-32 (inference only).  The module tree carries the reference's parameter and
    buffer names, so a checkpoint's ``model`` dict loads unchanged; ``unet.tf.*`` (the TimbreFilter, built but
    never called) and every ``num_batches_tracked`` are accepted and ignored.  ``forward`` runs pd_rmvpe_forward."""

    def __init__(self, n_blocks, n_gru, kernel_size, en_de_layers=5, inter_layers=4, in_channels=1, en_out_channels=16):
        super().__init__()
        if tuple(kernel_size) != (2, 2) or in_channels != 1:
            raise _lib.HipError("E2E0: only kernel_size (2, 2) and in_channels 1 are supported")
        self.config = dict(n_blocks=int(n_blocks), n_gru=int(n_gru), en_de_layers=int(en_de_layers),
                           inter_layers=int(inter_layers), en_out_channels=int(en_out_channels))
        self.param_keys = []
        for key, shape in synth.rmvpe_param_shapes(**self.config).items():
            stat = key.endswith(("running_mean", "running_var"))
            unit = synth._rmvpe_is_bn(key) and key.endswith(("weight", "running_var"))   # BatchNorm's own defaults
            init = torch.ones(shape) if unit else torch.zeros(shape)
            _attach(self, key, init, stat)
            self.param_keys.append(key)
        self._native = _lib.NativeHandle("E2E0", "pd_rmvpe_create", "pd_rmvpe_destroy", num_params="pd_rmvpe_num_params")
        self._ws = _lib.Workspace()
        self._compute_dtype = ("fp32", "fp32")      # (convs, recurrence)
        self._applied = None      # (handle, compute dtypes) of the last pd_rmvpe_set_option pair

    def set_compute_dtype(self, dtype, recurrence=None):
        """"fp32" (default) or "bf16".  ``dtype`` governs the 3x3 convs' operands (every conv but the first and
        ``cnn``), ``recurrence`` (default: ``dtype``) the GRU's recurrent product; activations, the gates, the input
        projection, the head and the decode stay fp32.  Takes effect at the next call; the handle is not rebuilt."""
        recurrence = dtype if recurrence is None else recurrence
        for v in (dtype, recurrence):
            if not isinstance(v, str) or v not in ("fp32", "bf16"):
                raise ValueError(f"E2E0: compute dtype must be 'fp32' or 'bf16', got {v!r}")
        self._compute_dtype = (dtype, recurrence)
        return self

    def load_state_dict(self, state_dict, strict=True, **kw):
        kept = {k: v for k, v in state_dict.items() if not synth.rmvpe_key_is_skipped(k)}
        return super().load_state_dict(kept, strict=strict, **kw)

    def dims(self):
        c = self.config
        return _lib.pd_rmvpe_dims(c["n_blocks"], c["n_gru"], c["en_de_layers"], c["inter_layers"], c["en_out_channels"],
                                  N_MELS, N_CLASS, synth.RMVPE_GRU_HIDDEN)

    def ordered_params(self):
        sd = dict(self.named_parameters())
        sd.update(dict(self.named_buffers()))
        return [sd[k] for k in self.param_keys]

    def handle(self):
        ps = self.ordered_params()
        h = self._native.get(self._native.signature(ps),
                             lambda: (self.dims(), [p.detach().float().contiguous() for p in ps]))
        want = (h.value, self._compute_dtype)
        if self._applied != want and (self._applied is not None or self._compute_dtype != ("fp32", "fp32")):
            L, st = _lib.lib(), _lib.stream_ptr(ps[0].device)
            for opt, v in zip((_lib.PD_RMVPE_OPT_CONV_DTYPE, _lib.PD_RMVPE_OPT_GRU_DTYPE), self._compute_dtype):
                _lib.check(L.pd_rmvpe_set_option(h, opt, _lib.PD_DTYPE_BF16 if v == "bf16" else _lib.PD_DTYPE_F32, st))
        self._applied = want
        return h

    def close(self):
        self._native.close()
        self._applied = None

    @torch.no_grad()
    def forward_time_major(self, mel_tm, return_feat=False, frames=None):
        """mel_tm [B, T, 128] time-major (what the native mel writes) -> hidden [B, T, 360] (and feat [B, T, 384]).
        ``frames``: a ragged batch's real frames per row, B host ints in [1, T] or a device int32 tensor
        (pd_rmvpe_forward_ragged): row b's first frames[b] output frames equal the row run alone, zero-padded to
        the multiple of 2^en_de_layers; what mel_tm holds past frames[b] is not used, the outputs there are
        unspecified."""
        mel_tm = mel_tm.float().contiguous()
        B, T, F = mel_tm.shape
        if F != N_MELS:
            raise ValueError(f"expected {N_MELS} mel bins, got {F}")
        h = self.handle()
        dev = mel_tm.device
        fr = None if frames is None else _lib._device_rows(frames, B, dev, "frames", 1, T)
        hidden = torch.empty(B, T, N_CLASS, device=dev, dtype=torch.float32)
        feat = torch.empty(B, T, 3 * N_MELS, device=dev, dtype=torch.float32) if return_feat else None
        L = _lib.lib()
        ws, wsb = self._ws.get(L.pd_rmvpe_workspace_size(h, B, T), dev)
        if fr is None:
            _lib.check(L.pd_rmvpe_forward(h, _lib.fptr(mel_tm), _lib.fptr(hidden), _lib.fptr(feat), B, T, ws, wsb,
                                          _lib.stream_ptr(dev)))
        else:
            _lib.check(L.pd_rmvpe_forward_ragged(h, _lib.fptr(mel_tm), _lib.iptr(fr), _lib.fptr(hidden), _lib.fptr(feat),
                                                 B, T, ws, wsb, _lib.stream_ptr(dev)))
        return (hidden, feat) if return_feat else hidden

    def forward(self, mel):
        """mel [B, 128, T] -> salience [B, T, 360]; T must be a multiple of 2^en_de_layers."""
        return self.forward_time_major(mel.transpose(1, 2))

    def forward_features(self, mel):
        """-> (hidden [B, T, 360], feat [B, T, 384]): ``feat`` is the ``cnn`` output as model.py:30 flattens it."""
        return self.forward_time_major(mel.transpose(1, 2), return_feat=True)


# ---------------------------------------------------------------- decode
@torch.no_grad()
def to_local_average_f0(hidden, center=None, thred=0.03):
    """modules/rmvpe/utils.py:8-23 on the GPU: hidden [B, T, n_class] -> f0 [B, T] (a device tensor; the
    reference's ``.squeeze(0).cpu().numpy()`` is left to the caller)."""
    hidden = hidden.float().contiguous()
    B, T, n = hidden.shape
    f0 = torch.empty(B, T, device=hidden.device, dtype=torch.float32)
    cen = None
    if center is not None:
        cen = center.to(hidden.device).long().reshape(B, T).contiguous()
    _lib.check(_lib.lib().pd_rmvpe_decode(_lib.fptr(hidden), _lib.fptr(f0), B, T, n, float(thred), _lib.lptr(cen),
                                          CONST, _lib.stream_ptr(hidden.device)))
    return f0


VITERBI_CHUNK = 32        # frames per backtrace chunk of pd_rmvpe_viterbi (PD_RMVPE_VITERBI_CHUNK)
_TINY = float(np.finfo(np.float32).tiny)      # librosa.util.tiny of a float32 probability
_VITERBI_TABLES = {}      # (n_class, width, device) -> (device log_band, log_off, log_init)
_VITERBI_WS = _lib.Workspace()


def viterbi_tables(n_class, width):
    """The transition of modules/rmvpe/utils.py:29-31 as librosa.sequence.viterbi takes its log, float64:
    (log_band [n_class, 2 width - 1] with lt[i][j] in column j - i + width - 1, log_off, log_init)."""
    i = np.arange(n_class)
    A = np.maximum(width - np.abs(i[:, None] - i[None, :]), 0)
    A = A / A.sum(axis=1, keepdims=True)
    lt = np.log(A + _TINY)
    log_off = float(np.log(0.0 + _TINY))
    band = np.full((n_class, 2 * width - 1), log_off)
    for c in range(2 * width - 1):
        j = i + c - (width - 1)
        ok = (j >= 0) & (j < n_class)
        band[i[ok], c] = lt[i[ok], j[ok]]
    return band, log_off, float(np.log(1.0 / n_class + _TINY))


@torch.no_grad()
def viterbi_path(hidden, width=30, return_logp=False, frames=None):
    """The path ``librosa.sequence.viterbi(prob, transition)`` finds for each row of hidden [B, T, n_class]
    (modules/rmvpe/utils.py:26-40, with the probabilities normalised in float64) on pd_rmvpe_viterbi:
    int64 [B, T] on hidden's device, and with ``return_logp`` the path's log-probability, float64 [B].  A frame
    that is zero in every class counts as uniform.  ``frames``: a ragged batch's frames per row (B host ints in
    [1, T] or a device int32 tensor, pd_rmvpe_viterbi_ragged): row b's path over its first frames[b] frames, as if
    decoded alone; the path is 0 past them, and what hidden holds there is not used."""
    if not hidden.is_cuda:
        raise _lib.HipError("viterbi_path runs on the GPU (got a CPU tensor; there is no CPU fallback)")
    hidden = hidden.float().contiguous()
    B, T, n = hidden.shape
    width = int(width)
    dev = hidden.device
    L = _lib.lib()
    if L.pd_rmvpe_viterbi_chunk() != VITERBI_CHUNK:
        raise _lib.HipError("VITERBI_CHUNK differs from the library's PD_RMVPE_VITERBI_CHUNK")
    key = (n, width, str(dev))
    tab = _VITERBI_TABLES.get(key)
    if tab is None:
        if torch.cuda.is_current_stream_capturing():
            raise _lib.HipError("viterbi_path: call once with this n_class and width before capturing a graph")
        band, log_off, log_init = viterbi_tables(n, width)
        tab = _VITERBI_TABLES[key] = (torch.from_numpy(band).to(dev), log_off, log_init)
    band, log_off, log_init = tab
    fr = None if frames is None else _lib._device_rows(frames, B, dev, "frames", 1, T)
    path = torch.empty(B, T, device=dev, dtype=torch.int64)
    logp = torch.empty(B, device=dev, dtype=torch.float64) if return_logp else None
    ws, wsb = _VITERBI_WS.get(L.pd_rmvpe_viterbi_workspace_size(B, T, n, width), dev)
    lp = None if logp is None else logp.data_ptr()
    if fr is None:
        _lib.check(L.pd_rmvpe_viterbi(_lib.fptr(hidden), band.data_ptr(), log_off, log_init, _lib.lptr(path), lp, B, T, n,
                                      width, ws, wsb, _lib.stream_ptr(dev)))
    else:
        _lib.check(L.pd_rmvpe_viterbi_ragged(_lib.fptr(hidden), band.data_ptr(), log_off, log_init, _lib.lptr(path), lp,
                                             _lib.iptr(fr), B, T, n, width, ws, wsb, _lib.stream_ptr(dev)))
    return (path, logp) if return_logp else path


@torch.no_grad()
def to_viterbi_f0(hidden, thred=0.03, frames=None):
    """modules/rmvpe/utils.py:26-43 on the GPU, for any batch size: hidden [B, T, n_class] -> f0 [B, T] (device).
    ``frames``: as in ``viterbi_path``; f0 past a row's own frames is unspecified."""
    return to_local_average_f0(hidden, center=viterbi_path(hidden, frames=frames), thred=thred)


def resampled_length(n, original_timestep, target_timestep):
    """len(np.arange(0, (n - 1) * original_timestep, target_timestep)) without building the array."""
    return int(np.ceil((n - 1) * original_timestep / target_timestep))


@torch.no_grad()
def align_rows(frames, length, original_timestep, target_timestep, n_max=None):
    """The (n_b, m_b, length_b) rows of a ragged ``align_f0`` from host values, checked as pd_f0_align checks its
    own: ``frames`` B ints (source frames per row), ``length`` an int or B ints -> list of B triples."""
    frames = [int(v) for v in frames]
    B = len(frames)
    lengths = [int(length)] * B if np.ndim(length) == 0 else [int(v) for v in length]
    if len(lengths) != B:
        raise _lib.HipError(f"length holds {len(lengths)} values for a batch of {B}")
    rows = []
    for b, (n, ln) in enumerate(zip(frames, lengths)):
        m = resampled_length(n, float(original_timestep), float(target_timestep)) if n >= 2 else 0
        if n < 2 or m < 1 or ln < 1 or (n_max is not None and n > n_max):
            raise ValueError(f"align_f0 needs two source frames, one resampled frame and a positive length (row {b}: "
                             f"n = {n}, resampled {m}, length {ln})")
        rows.append((n, m, ln))
    return rows


@torch.no_grad()
def align_f0(f0, original_timestep, target_timestep, length, interp_uv=False, frames=None):
    """``RMVPE.get_pitch`` after ``infer_from_audio``, on the GPU (pd_f0_align): f0 [B, n] (or [n]) at
    ``original_timestep`` -> (f0 float32 [B, length], uv bool [B, length]) at ``target_timestep``, both on the
    device: interp_f0, resample_align_curve of the curve and of uv, uv > 0.5, and f0 = 0 where unvoiced unless
    ``interp_uv``.

    Ragged (pd_f0_align_ragged), when ``frames`` is given or ``length`` holds B ints: row b is its first
    frames[b] source frames (default n) aligned onto length[b] frames; the outputs are [B, max(length)] with
    f0 = 0 and uv = True past a row's own length.  ``frames`` is B host ints (each row's resampled length is
    worked out on the host, the triples go up as one small cached copy), or a device int32 tensor [B, 3] of
    (n_b, m_b, length_b) as ``align_rows`` gives them, with ``length`` the int width of the outputs."""
    if not f0.is_cuda:
        raise _lib.HipError("align_f0 runs on the GPU (got a CPU tensor; there is no CPU fallback)")
    single = f0.dim() == 1
    f0 = f0.float().reshape(-1, f0.shape[-1]).contiguous()
    B, n = f0.shape
    if frames is not None or np.ndim(length) != 0:
        if torch.is_tensor(frames) and frames.is_cuda:
            if tuple(frames.shape) != (B, 3) or np.ndim(length) != 0:
                raise _lib.HipError("align_f0: a device `frames` is int32 [B, 3] (n, m, length) and needs an int `length`")
            width = int(length)
            rows = frames if frames.dtype == torch.int32 and frames.is_contiguous() else frames.to(torch.int32).contiguous()
        else:
            host = [n] * B if frames is None else (frames.tolist() if torch.is_tensor(frames) else list(frames))
            if len(host) != B:
                raise _lib.HipError(f"frames holds {len(host)} values for a batch of {B}")
            triples = align_rows(host, length, original_timestep, target_timestep, n_max=n)
            width = max(t[2] for t in triples)
            rows = _lib._device_rows([v for t in triples for v in t], 3 * B, f0.device, "f0_rows", 1, 2 ** 31 - 1)
        if n < 2 or width < 1:
            raise ValueError(f"align_f0 needs two source frames and a positive length (n = {n}, length {width})")
        out = torch.empty(B, width, device=f0.device, dtype=torch.float32)
        uv = torch.empty(B, width, device=f0.device, dtype=torch.bool)
        _lib.check(_lib.lib().pd_f0_align_ragged(_lib.fptr(f0), _lib.fptr(out), uv.data_ptr(), _lib.iptr(rows), B, n, width,
                                                 float(original_timestep), float(target_timestep), int(bool(interp_uv)),
                                                 _lib.stream_ptr(f0.device)))
        return (out[0], uv[0]) if single else (out, uv)
    length = int(length)
    m = resampled_length(n, float(original_timestep), float(target_timestep)) if n >= 2 else 0
    if n < 2 or m < 1 or length < 1:
        raise ValueError(f"align_f0 needs two source frames, one resampled frame and a positive length (n = {n}, "
                         f"resampled {m}, length {length})")
    out = torch.empty(B, length, device=f0.device, dtype=torch.float32)
    uv = torch.empty(B, length, device=f0.device, dtype=torch.bool)
    _lib.check(_lib.lib().pd_f0_align(_lib.fptr(f0), _lib.fptr(out), uv.data_ptr(), B, n, m, length, float(original_timestep),
                                      float(target_timestep), int(bool(interp_uv)), _lib.stream_ptr(f0.device)))
    return (out[0], uv[0]) if single else (out, uv)


# ---------------------------------------------------------------- front end
class MelSpectrogram(MelFrontEnd):
    """modules/rmvpe/spec.py: the HTK-scale log-mel of ``torch.stft(center=True)`` on the centred pd_mel.
    ``forward`` returns the reference's [B, n_mels, T] (a transposed view of the time-major native output,
    which ``forward_time_major`` returns as it is); T = 1 + L // hop."""

    def __init__(self, n_mel_channels, sampling_rate, win_length, hop_length, n_fft=None, mel_fmin=0, mel_fmax=None,
                 clamp=1e-5):
        self.n_fft = win_length if n_fft is None else n_fft
        self.n_mel_channels, self.sampling_rate = n_mel_channels, sampling_rate
        self.win_length, self.hop_length, self.clamp = win_length, hop_length, clamp
        basis = mel_filterbank(sampling_rate, self.n_fft, n_mel_channels, mel_fmin, mel_fmax, htk=True)
        self._setup("MelSpectrogram", "pd_mel_create_centered", basis, self.n_fft, win_length, hop_length, clamp)

    def to(self, device):
        return self

    def _min_samples(self, keyshift, speed):
        nf = derived_sizes(self.n_fft, self.win_length, self.hop_length, keyshift, speed)[0]
        return nf // 2 + 1, "reflect padding needs"

    def forward_time_major(self, audio, keyshift=0, speed=1, center=True, return_spec=False, lens=None):
        if not center:
            raise NotImplementedError("center=False is prodiff_amd.mel.STFT's framing")
        return self._mel_time_major(audio, keyshift, speed, lens=lens, return_spec=return_spec)

    def forward(self, audio, keyshift=0, speed=1, center=True):
        return self.forward_time_major(audio, keyshift, speed, center).transpose(1, 2)

    __call__ = forward


# ---------------------------------------------------------------- curves (utils/pitch_utils.py)
def interp_f0(f0, uv=None):
    """utils/pitch_utils.py:45-51: unvoiced frames filled by linear interpolation of log2 f0 -> (f0, uv)."""
    f0 = np.asarray(f0)
    if uv is None:
        uv = f0 == 0
    with np.errstate(divide="ignore"):
        lf = np.log2(f0 + uv)
    lf[uv] = -np.inf
    if uv.any() and not uv.all():
        lf[uv] = np.interp(np.where(uv)[0], np.where(~uv)[0], lf[~uv])
    return 2 ** lf, uv


def resample_align_curve(points, original_timestep, target_timestep, align_length):
    """utils/pitch_utils.py:86-98: the curve at another frame period, cut or padded (last value) to align_length."""
    points = np.asarray(points)
    t_max = (len(points) - 1) * original_timestep
    curve = np.interp(np.arange(0, t_max, target_timestep), original_timestep * np.arange(len(points)),
                      points).astype(points.dtype)
    delta_l = align_length - len(curve)
    if delta_l < 0:
        curve = curve[:align_length]
    elif delta_l > 0:
        curve = np.concatenate((curve, np.full(delta_l, fill_value=curve[-1], dtype=curve.dtype)), axis=0)
    return curve


# ---------------------------------------------------------------- ragged batches
MIN_SAMPLES_16K = WINDOW_LENGTH // 2 + 1      # the centred mel's reflect padding (pd_mel_min_samples)


def pitch_row_sizes(lens, samplerate, hop_length=160):
    """The per-row sizes of a ragged ``get_pitch_batch`` from the rows' sample counts, on the host:
    (samples at 16 kHz = pd_resample_out_samples, mel frames T_b = 1 + L16_b // hop, T = the longest row's frames
    padded to a multiple of 32).  A row below the centred mel's minimum raises ValueError."""
    g = int(np.gcd(int(samplerate), SAMPLE_RATE))
    o, n = int(samplerate) // g, SAMPLE_RATE // g
    lens16 = [-(-n * int(v) // o) for v in lens]
    for b, v in enumerate(lens16):
        if v < MIN_SAMPLES_16K:
            raise ValueError(f"row {b}: {int(lens[b])} samples at {samplerate} Hz are {v} at {SAMPLE_RATE} Hz, the centred "
                             f"mel needs at least {MIN_SAMPLES_16K}")
    frames = [1 + v // hop_length for v in lens16]
    return lens16, frames, 32 * ((max(frames) - 1) // 32 + 1)


def stack_waveforms(waveforms, lens, device):
    """A ragged batch as (float32 [B, L_max] on the device, B host sample counts): a list or tuple of 1-D arrays
    or tensors stacked into one zero-padded copy, or a padded [B, L] with ``lens``."""
    if isinstance(waveforms, (list, tuple)) and lens is None:
        rows = [w if torch.is_tensor(w) else torch.from_numpy(np.asarray(w)) for w in waveforms]
        if not rows or any(r.dim() != 1 for r in rows):
            raise ValueError("a ragged batch is a non-empty list of 1-D waveforms")
        lens = [int(r.shape[0]) for r in rows]
        if any(r.is_cuda for r in rows):
            audio = torch.zeros(len(rows), max(lens), device=device, dtype=torch.float32)
        else:
            audio = torch.zeros(len(rows), max(lens), dtype=torch.float32)
            if torch.device(device).type == "cuda":
                audio = audio.pin_memory()
        for b, r in enumerate(rows):
            audio[b, :lens[b]] = r
        return audio.to(device, non_blocking=True), lens
    audio = waveforms if torch.is_tensor(waveforms) else torch.from_numpy(np.asarray(waveforms))
    audio = audio.float().reshape(-1, audio.shape[-1]).to(device)
    B, L = audio.shape
    if lens is None:
        lens = [L] * B
    elif torch.is_tensor(lens) and lens.is_cuda:
        raise _lib.HipError("get_pitch_batch: `lens` must be host integers (the per-row sizes are worked out on the host)")
    lens = [int(v) for v in (lens.tolist() if torch.is_tensor(lens) else lens)]
    if len(lens) != B or min(lens) < 1 or max(lens) > L:
        raise _lib.HipError(f"lens must hold {B} values in [1, {L}]")
    return audio, lens


# ---------------------------------------------------------------- extractor
@register_pe
class RMVPE:
    """component/pe/rmvpe.py:13-72.  ``model_path=None`` with no ``pe_ckpt`` in hparams builds the model without
    weights (load them with ``self.model.load_state_dict``).  ``compute_dtype``: ``E2E0.set_compute_dtype``."""

    def __init__(self, hparams, model_path=None, hop_length=160, compute_dtype="fp32"):
        self.hparams = hparams
        self.resample_kernel = {}
        self.device = "cuda"
        self.model = E2E0(4, 1, (2, 2)).eval().to(self.device)
        if model_path is None:
            model_path = (hparams or {}).get("pe_ckpt")
        if model_path is not None:
            ckpt = torch.load(model_path, map_location=self.device)
            self.model.load_state_dict(ckpt["model"], strict=False)
        self.mel_extractor = MelSpectrogram(N_MELS, SAMPLE_RATE, WINDOW_LENGTH, hop_length, None, MEL_FMIN, MEL_FMAX)
        self.set_compute_dtype(compute_dtype)

    def set_compute_dtype(self, dtype, recurrence=None):
        """``E2E0.set_compute_dtype`` of the model; returns self."""
        self.model.set_compute_dtype(dtype, recurrence)
        return self

    @torch.no_grad()
    def mel2hidden(self, mel, frames=None):
        """mel [B, 128, T] -> hidden [B, T, 360]: zero-padded (value 0.0, real network input) to a multiple of 32.
        ``frames``: a ragged batch's real frames per row (``E2E0.forward_time_major``); T, the longest row's, is
        what gets padded, each row is computed as if padded to its own multiple of 32."""
        return self._hidden_time_major(mel.transpose(1, 2), frames=frames)

    def _hidden_time_major(self, mel_tm, frames=None):
        n_frames = mel_tm.shape[1]
        pad = 32 * ((n_frames - 1) // 32 + 1) - n_frames
        if pad:
            mel_tm = torch.nn.functional.pad(mel_tm, (0, 0, 0, pad))
        return self.model.forward_time_major(mel_tm, frames=frames)[:, :n_frames]

    def decode(self, hidden, thred=0.03, use_viterbi=False):
        if use_viterbi:
            if not hidden.is_cuda:
                raise NotImplementedError("Viterbi decoding runs on the GPU: pass a device tensor (librosa on the CPU, "
                                          "as in the reference, is not offered)")
            return to_viterbi_f0(hidden, thred=thred).squeeze(0).cpu().numpy()
        return to_local_average_f0(hidden, thred=thred).squeeze(0).cpu().numpy()

    def _hidden_from_audio(self, audio, sample_rate, lens=None, lens16=None, frames=None):
        """audio [B, L] on the device at ``sample_rate`` -> hidden [B, T, 360]: resampler, centred mel, network.
        Ragged: ``lens`` samples per row, ``lens16`` / ``frames`` the same rows at 16 kHz / in mel frames
        (``pitch_row_sizes``); T is the longest row's."""
        if sample_rate != SAMPLE_RATE:
            key = str(sample_rate)
            if key not in self.resample_kernel:
                self.resample_kernel[key] = Resample(sample_rate, SAMPLE_RATE, lowpass_filter_width=128)
            audio = self.resample_kernel[key](audio, lens=lens)
        mel_tm = self.mel_extractor.forward_time_major(audio, center=True, lens=lens16)
        if frames is not None:
            mel_tm = mel_tm[:, :max(frames)]
        return self._hidden_time_major(mel_tm, frames=frames)

    def infer_from_audio(self, audio, sample_rate=16000, thred=0.03, use_viterbi=False):
        audio = torch.from_numpy(np.asarray(audio)).float().unsqueeze(0).to(self.device)
        return self.decode(self._hidden_from_audio(audio, sample_rate), thred=thred, use_viterbi=use_viterbi)

    @torch.no_grad()
    def get_pitch_batch(self, waveforms, samplerate, length, *, lens=None, hop_size, speed=1, interp_uv=False,
                        use_viterbi=False, thred=0.03):
        """``get_pitch`` for a batch of waveforms, entirely on the device: -> (f0 float32 [B, length], uv bool
        [B, length]) as device tensors.  Everything after the waveforms' copy to the device is stream-ordered;
        nothing waits on the host and nothing is read back.

        ``waveforms`` is [B, L] (device or host) of equally long rows, or a ragged batch: a list or tuple of
        1-D arrays or tensors of any lengths (stacked into one zero-padded [B, L_max] copy to the device), or a
        padded [B, L] with ``lens`` (B host ints, samples per row).  ``length`` is an int or B ints.  Each row of
        a ragged batch equals that clip run alone; the outputs are [B, max(length)] with f0 = 0 and uv = True
        past a row's own length.  A row too short for the centred mel raises ValueError."""
        time_step = int(np.round(hop_size * speed)) / samplerate
        if isinstance(waveforms, (list, tuple)) or lens is not None or np.ndim(length) != 0:
            audio, lens = stack_waveforms(waveforms, lens, self.device)
            lens16, frames, _ = pitch_row_sizes(lens, samplerate)
            rows = align_rows(frames, length, 0.01, time_step)          # checked before anything is launched
            hidden = self._hidden_from_audio(audio, samplerate, lens, lens16, frames)
            f0 = to_viterbi_f0(hidden, thred, frames) if use_viterbi else to_local_average_f0(hidden, thred=thred)
            return align_f0(f0, 0.01, time_step, [r[2] for r in rows], interp_uv=interp_uv, frames=frames)
        audio = waveforms if torch.is_tensor(waveforms) else torch.from_numpy(np.asarray(waveforms))
        audio = audio.float().reshape(-1, audio.shape[-1]).to(self.device)
        hidden = self._hidden_from_audio(audio, samplerate)
        f0 = to_viterbi_f0(hidden, thred=thred) if use_viterbi else to_local_average_f0(hidden, thred=thred)
        return align_f0(f0, 0.01, time_step, length, interp_uv=interp_uv)

    def get_pitch(self, waveform, samplerate, length, *, hop_size, f0_min=65, f0_max=1100, speed=1, interp_uv=False,
                  use_viterbi=False, thred=0.03):
        f0 = self.infer_from_audio(waveform, sample_rate=samplerate, thred=thred, use_viterbi=use_viterbi)
        uv = f0 == 0
        f0, uv = interp_f0(f0, uv)
        hop_size = int(np.round(hop_size * speed))
        time_step = hop_size / samplerate
        f0_res = resample_align_curve(f0, 0.01, time_step, length)
        uv_res = resample_align_curve(uv.astype(np.float32), 0.01, time_step, length) > 0.5
        if not interp_uv:
            f0_res[uv_res] = 0
        return f0_res, uv_res
