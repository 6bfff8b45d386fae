"""Harmonic-noise separation on the GPU: the reference's modules/vr (``CascadedNet``, ``load_sep_model``) and
component/binarizer/binarizer_utils.py ``extract_harmonic_aperiodic`` on pd_vr (include/prodiff_hip.h, "harmonic-noise
separation").  Inference only.  fp32 is the default; ``set_compute_dtype("bf16")`` runs every conv but the last
on the bf16 MFMA (PD_VR_OPT_CONV_DTYPE), all else staying fp32.
"""
from __future__ import annotations

import pathlib

import numpy as np
import torch
from torch import nn

from . import _lib, synth
from .rmvpe import _attach, stack_waveforms

MAX_LSTM_HIDDEN = 64      # per direction: what the recurrence kernel holds (pd_vr_dims.nout_lstm <= 128)


def padded_frames(n_samples, hop_length):
    """nets.py:178-181: (T, Tl_pad, T_pad) of ``predict_from_audio`` -- a frame count that is already a multiple
    of 32 gains a whole extra 32 frames."""
    n_frames = n_samples // hop_length + 1
    T = 32 * (n_frames // 32 + 1)
    T_pad = (T - 1) * hop_length - n_samples
    Tl_pad = T_pad // 2 // hop_length * hop_length
    return T, Tl_pad, T_pad


def row_sizes(lens, n_fft, hop_length):
    """The per-row sizes of a ragged batch from the rows' sample counts, on the host: a list of
    (T_b, lead_b) = (pd_vr_frames, pd_vr_lead) per row, which the kernels restate from ``lens``."""
    out = []
    for n in lens:
        T, Tl_pad, _ = padded_frames(int(n), hop_length)
        out.append((T, n_fft // 2 + Tl_pad))
    return out


def check_dims(n_fft, hop_length, nout, nout_lstm):
    """The dimensions pd_vr_create takes; raises HipError naming the first one outside them."""
    if n_fft % 64 != 0 or not 64 <= n_fft <= 16384:
        raise _lib.HipError(f"CascadedNet: n_fft must be a multiple of 64 in [64, 16384], got {n_fft}")
    if hop_length < 16 or n_fft % hop_length != 0 or hop_length == n_fft:
        raise _lib.HipError(f"CascadedNet: hop_length must be >= 16 and a proper divisor of n_fft, got {hop_length}")
    if nout % 4 != 0 or not 4 <= nout <= 256:
        raise _lib.HipError(f"CascadedNet: nout must be a multiple of 4 in [4, 256], got {nout}")
    if nout_lstm % 2 != 0:
        raise _lib.HipError(f"CascadedNet: nout_lstm must be even, got {nout_lstm}")
    if nout_lstm % 4 != 0 or nout_lstm < 4:
        raise _lib.HipError(f"CascadedNet: the high-band nets split nout_lstm / 2 over two directions: nout_lstm must "
                            f"be a positive multiple of 4, got {nout_lstm}")
    if nout_lstm // 2 > MAX_LSTM_HIDDEN:
        raise _lib.HipError(f"CascadedNet: the recurrence kernel holds {MAX_LSTM_HIDDEN} hidden units per direction "
                            f"(nout_lstm <= {2 * MAX_LSTM_HIDDEN}), got nout_lstm {nout_lstm}")


def _planar(spec):
    """complex [B, C, F, T] -> (re, im) float32 [B * C, T, F] contiguous."""
    B, Cn, F, T = spec.shape
    v = torch.view_as_real(spec.to(torch.complex64)).reshape(B * Cn, F, T, 2).permute(3, 0, 2, 1).contiguous()
    return v[0], v[1]


def _complex(re, im, B, Cn):
    """(re, im) [B * C, T, F] -> complex64 [B, C, F, T]."""
    rows, T, F = re.shape
    return torch.complex(re, im).reshape(B, Cn, T, F).transpose(2, 3)


class CascadedNet(nn.Module):
    """modules/vr/nets.py:44-197 (inference only).  The module tree carries the reference's parameter and buffer
    names, so ``load_state_dict(torch.load(model.pt))`` works unchanged; every ``num_batches_tracked`` is accepted
    and ignored, ``aux_out`` (a training-time head) is kept and not read, ``window`` is a non-persistent buffer."""

    def __init__(self, n_fft, hop_length, nout=32, nout_lstm=128, is_complex=True, is_mono=False):
        super().__init__()
        if not is_complex:
            raise _lib.HipError("CascadedNet: only is_complex=True is supported (what load_sep_model builds)")
        check_dims(n_fft, hop_length, nout, nout_lstm)
        self.n_fft, self.hop_length = int(n_fft), int(hop_length)
        self.nout, self.nout_lstm = int(nout), int(nout_lstm)
        self.is_complex, self.is_mono = True, bool(is_mono)
        self.max_bin = n_fft // 2
        self.output_bin = n_fft // 2 + 1
        self.nin_lstm = self.max_bin // 2
        self.offset = 64
        self.channels = 1 if is_mono else 2
        self.param_keys = []
        for key, shape in synth.vr_param_shapes(n_fft, nout, nout_lstm, is_mono).items():
            stat = key.endswith(("running_mean", "running_var"))
            unit = synth.vr_is_bn(key) and key.endswith(("weight", "running_var"))   # BatchNorm's own defaults
            _attach(self, key, torch.ones(shape) if unit else torch.zeros(shape), stat)
            self.param_keys.append(key)
        self.register_buffer("window", torch.hann_window(n_fft), persistent=False)
        self._native = _lib.NativeHandle("CascadedNet", "pd_vr_create", "pd_vr_destroy", num_params="pd_vr_num_params")
        self._ws = _lib.Workspace()
        self._compute_dtype = "fp32"
        self._applied = None      # (handle, compute dtype) of the last pd_vr_set_option

    def set_compute_dtype(self, dtype):
        """"fp32" (default) or "bf16": the convs' operands (every conv but ``out``); activations, the LSTM, the
        transforms and the mask stay fp32.  Takes effect at the next call; the handle is not rebuilt."""
        if dtype not in ("fp32", "bf16"):
            raise ValueError(f"CascadedNet: compute dtype must be 'fp32' or 'bf16', got {dtype!r}")
        self._compute_dtype = dtype
        return self

    def load_state_dict(self, state_dict, strict=True, **kw):
        kept = {k: v for k, v in state_dict.items() if not k.endswith("num_batches_tracked")}
        return super().load_state_dict(kept, strict=strict, **kw)

    def dims(self):
        return _lib.pd_vr_dims(self.n_fft, self.hop_length, self.nout, self.nout_lstm, int(self.is_mono))

    def ordered_params(self):
        sd = dict(self.named_parameters())
        sd.update(dict(self.named_buffers()))
        return [sd[k] for k in self.param_keys] + [self.window]

    def handle(self):
        ps = self.ordered_params()
        h = self._native.get(self._native.signature(ps),
                             lambda: (self.dims(), [p.detach().float().contiguous() for p in ps]))
        want = (h.value, self._compute_dtype)
        if self._applied != want and (self._applied is not None or self._compute_dtype != "fp32"):
            dt = _lib.PD_DTYPE_BF16 if self._compute_dtype == "bf16" else _lib.PD_DTYPE_F32
            _lib.check(_lib.lib().pd_vr_set_option(h, _lib.PD_VR_OPT_CONV_DTYPE, dt, _lib.stream_ptr(ps[0].device)))
        self._applied = want
        return h

    def close(self):
        self._native.close()
        self._applied = None

    # ---------------------------------------------------------------- the three stages on planar spectra
    def _check_wav(self, x):
        if x.dim() != 3 or x.shape[1] != self.channels:
            raise ValueError(f"expected a [B, {self.channels}, L] waveform, got {tuple(x.shape)}")
        return x.float().contiguous()

    def _lens(self, lens, B, L, dev, name="lens"):
        """A ragged batch's sample counts, B host ints in [1, L] -> (the ints, a cached device int32 copy)."""
        if torch.is_tensor(lens) and lens.is_cuda:
            raise _lib.HipError(f"CascadedNet: `{name}` must be host integers (the per-row sizes are worked out on the "
                                "host)")
        host = [int(v) for v in (lens.tolist() if torch.is_tensor(lens) else lens)]
        return host, _lib._device_rows(host, B, dev, name, 1, L)

    def _stft(self, rows, lead, T, lens=None):
        """rows [R, L] -> (re, im) [R, T, n_fft/2 + 1]; frame t covers samples [t hop - lead, .. + n_fft).
        ``lens`` (R host ints): a ragged batch (pd_vr_stft_ragged) -- row r is its first lens[r] samples with its
        own frame count and lead (``lead`` is not used), its frames past that count stay zero."""
        h = self.handle()
        R, L = rows.shape
        if lens is not None:
            _, ld = self._lens(lens, R, L, rows.device)
            re = torch.zeros(R, T, self.output_bin, device=rows.device, dtype=torch.float32)
            im = torch.zeros_like(re)
            _lib.check(_lib.lib().pd_vr_stft_ragged(h, _lib.fptr(rows), _lib.iptr(ld), _lib.fptr(re), _lib.fptr(im), R, L,
                                                    T, _lib.stream_ptr(rows.device)))
            return re, im
        re = torch.empty(R, T, self.output_bin, device=rows.device, dtype=torch.float32)
        im = torch.empty_like(re)
        _lib.check(_lib.lib().pd_vr_stft(h, _lib.fptr(rows), _lib.fptr(re), _lib.fptr(im), R, L, lead, T,
                                         _lib.stream_ptr(rows.device)))
        return re, im

    def _mask(self, re, im, B, frames=None):
        """``frames`` (B host ints, positive multiples of 32 up to T): a ragged batch (pd_vr_mask_ragged); the
        mask past a row's frames is unspecified."""
        h = self.handle()
        R, T, F = re.shape
        if R != B * self.channels or F != self.output_bin:
            raise ValueError(f"expected a spectrum of {self.channels} channels and {self.output_bin} bins")
        if T % 32 != 0:
            raise ValueError(f"the frame count must be a multiple of 32 (crop_center is not implemented), got {T}")
        L = _lib.lib()
        mre, mim = torch.empty_like(re), torch.empty_like(im)
        ws, wsb = self._ws.get(L.pd_vr_workspace_size(h, B, (T - 32) * self.hop_length), re.device)
        if frames is not None:
            if torch.is_tensor(frames) and frames.is_cuda:
                raise _lib.HipError("CascadedNet: `frames` must be host integers")
            host = [int(v) for v in (frames.tolist() if torch.is_tensor(frames) else frames)]
            if any(v % 32 != 0 for v in host):
                raise _lib.HipError(f"frames must be positive multiples of 32, got {host}")
            fd = _lib._device_rows(host, B, re.device, "frames", 32, T)
            _lib.check(L.pd_vr_mask_ragged(h, _lib.fptr(re), _lib.fptr(im), _lib.iptr(fd), _lib.fptr(mre), _lib.fptr(mim),
                                           B, T, ws, wsb, _lib.stream_ptr(re.device)))
            return mre, mim
        _lib.check(L.pd_vr_mask(h, _lib.fptr(re), _lib.fptr(im), _lib.fptr(mre), _lib.fptr(mim), B, T, ws, wsb,
                                _lib.stream_ptr(re.device)))
        return mre, mim

    def _istft(self, re, im, mre, mim, lead, L_out, wav=None, lens=None):
        """-> y [R, L_out] (and wav - y when ``wav`` [R, L_out] is given, from the same epilogue).  ``lens``
        (R host ints): a ragged batch (pd_vr_istft_ragged) -- row r's first lens[r] samples from its own frames and
        lead (``lead`` is not used), zeros from there to L_out."""
        h = self.handle()
        R, T, _ = re.shape
        y = torch.empty(R, L_out, device=re.device, dtype=torch.float32)
        resid = torch.empty_like(y) if wav is not None else None
        if lens is not None:
            _, ld = self._lens(lens, R, L_out, re.device)
            _lib.check(_lib.lib().pd_vr_istft_ragged(h, _lib.fptr(re), _lib.fptr(im), _lib.fptr(mre), _lib.fptr(mim),
                                                     _lib.fptr(wav), _lib.iptr(ld), _lib.fptr(y), _lib.fptr(resid), R, T,
                                                     L_out, _lib.stream_ptr(re.device)))
            return (y, resid) if wav is not None else y
        _lib.check(_lib.lib().pd_vr_istft(h, _lib.fptr(re), _lib.fptr(im), _lib.fptr(mre), _lib.fptr(mim), _lib.fptr(wav),
                                          _lib.fptr(y), _lib.fptr(resid), R, T, lead, L_out, _lib.stream_ptr(re.device)))
        return (y, resid) if wav is not None else y

    # ---------------------------------------------------------------- the reference's methods
    @torch.no_grad()
    def forward(self, x):
        """spectrum complex [B, C, n_fft/2 + 1, T] -> mask complex [B, C, n_fft/2 + 1, T]; T a multiple of 32."""
        B, Cn = x.shape[:2]
        re, im = _planar(x)
        mre, mim = self._mask(re, im, B)
        return _complex(mre, mim, B, Cn)

    def predict_mask(self, x):
        mask = self.forward(x)
        if self.offset > 0:
            mask = mask[:, :, :, self.offset:-self.offset]
            assert mask.size()[3] > 0
        return mask

    def predict(self, x):
        pred = x * self.forward(x)
        if self.offset > 0:
            pred = pred[:, :, :, self.offset:-self.offset]
            assert pred.size()[3] > 0
        return pred

    @torch.no_grad()
    def audio2spec(self, x, use_pad=False):
        """nets.py:149-166: [B, C, L] -> complex [B, C, n_fft/2 + 1, T]."""
        x = self._check_wav(x)
        B, Cn, L = x.shape
        n_frames = L // self.hop_length + 1
        T, Tl_pad = n_frames, 0
        if use_pad:
            T = 32 * ((n_frames - 1) // 32 + 1)
            Tl_pad = ((T - 1) * self.hop_length - L) // 2 // self.hop_length * self.hop_length
        re, im = self._stft(x.reshape(B * Cn, L), self.n_fft // 2 + Tl_pad, T)
        return _complex(re, im, B, Cn)

    @torch.no_grad()
    def spec2audio(self, x):
        """nets.py:168-173: complex [B, C, n_fft/2 + 1, T] -> [B, C, (T - 1) hop]."""
        B, Cn, _, T = x.shape
        re, im = _planar(x)
        return self._istft(re, im, None, None, self.n_fft // 2, (T - 1) * self.hop_length).reshape(B, Cn, -1)

    @torch.no_grad()
    def separate(self, wav, lens=None):
        """[B, C, L] -> (harmonic, aperiodic = wav - harmonic), both [B, C, L], in one pd_vr_separate call.
        ``lens`` (B host ints in [1, L]): a ragged batch (pd_vr_separate_ragged) -- row b's first lens[b] samples
        equal, bit for bit, that clip run alone; what ``wav`` holds past them is not used, the outputs there are 0."""
        x = self._check_wav(wav)
        B, Cn, L = x.shape
        h = self.handle()
        lib = _lib.lib()
        ld = None if lens is None else self._lens(lens, B, L, x.device)[1]
        y, ap = torch.empty_like(x), torch.empty_like(x)
        ws, wsb = self._ws.get(lib.pd_vr_workspace_size(h, B, L), x.device)
        if ld is not None:
            _lib.check(lib.pd_vr_separate_ragged(h, _lib.fptr(x), _lib.iptr(ld), _lib.fptr(y), _lib.fptr(ap), B, L, ws,
                                                 wsb, _lib.stream_ptr(x.device)))
            return y, ap
        _lib.check(lib.pd_vr_separate(h, _lib.fptr(x), _lib.fptr(y), _lib.fptr(ap), B, L, ws, wsb,
                                      _lib.stream_ptr(x.device)))
        return y, ap

    def predict_from_audio(self, x, lens=None):
        """nets.py:175-197: [B, C, L] -> the harmonic part [B, C, L]; ``lens``: a ragged batch (``separate``)."""
        return self.separate(x, lens)[0]


def load_sep_model(model_path, device="cuda", *, compute_dtype="fp32"):
    """modules/vr/__init__.py:18-35: the model described by ``config.yaml`` beside the checkpoint;
    ``compute_dtype``: ``CascadedNet.set_compute_dtype``."""
    import yaml
    model_path = pathlib.Path(model_path)
    with open(model_path.with_name("config.yaml"), "r") as f:
        args = yaml.safe_load(f)
    model = CascadedNet(args["n_fft"], args["hop_length"], args["n_out"], args["n_out_lstm"], True,
                        is_mono=args["is_mono"])
    model.load_state_dict(torch.load(model_path, map_location="cpu", weights_only=True))
    return model.to(device).eval().set_compute_dtype(compute_dtype)


SEP_MODEL = None


def extract_harmonic_aperiodic(waveform, model_path=None, device="cuda"):
    """component/binarizer/binarizer_utils.py:99-113: a mono waveform (numpy [L]) -> (harmonic, aperiodic) numpy [L].  The model is
    loaded on the first call and kept at module level, as in the reference; ``model_path`` may also be a
    ``CascadedNet``.  A list or tuple of mono waveforms of different lengths goes through one ragged
    ``separate`` call and gives a list of (harmonic, aperiodic), each pair what its clip gives alone.  The model's
    own compute dtype (``set_compute_dtype``) applies."""
    global SEP_MODEL
    if isinstance(model_path, CascadedNet):
        model = model_path
    else:
        if SEP_MODEL is None:
            SEP_MODEL = load_sep_model(model_path, device)
        model = SEP_MODEL
    dev = next(model.parameters()).device
    if isinstance(waveform, (list, tuple)):
        audio, lens = stack_waveforms(waveform, None, dev)
        x = audio[:, None]
        y, ap = model.separate(x if model.is_mono else x.repeat(1, 2, 1), lens)
        out = []
        for b, n in enumerate(lens):
            if model.is_mono:
                harmonic, aperiodic = y[b, 0, :n], ap[b, 0, :n]
            else:
                harmonic = y[b, :, :n].mean(dim=0)
                aperiodic = audio[b, :n] - harmonic
            out.append((harmonic.cpu().numpy(), aperiodic.cpu().numpy()))
        return out
    wav = torch.from_numpy(np.asarray(waveform, dtype=np.float32)).to(dev)
    x = wav[None, None]
    if not model.is_mono:
        x = x.repeat(1, 2, 1)
    y, ap = model.separate(x)
    if model.is_mono:
        harmonic, aperiodic = y[0, 0], ap[0, 0]
    else:
        harmonic = y[0].mean(dim=0)
        aperiodic = wav - harmonic
    return harmonic.cpu().numpy(), aperiodic.cpu().numpy()
