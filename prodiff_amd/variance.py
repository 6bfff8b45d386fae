"""Pitch and duration predictors with their encoders on the GPU, drop-ins for the reference.

``PitchPredictor`` replaces modules/variance_predictor/pitch_predictor.py:10-121 and
``DurPredictor`` replaces modules/variance_predictor/dur_predictor.py:7-36: the same
constructors ``(vocab_size, hparams)``, child modules and state-dict keys
(``encoder.layers.N.op.*``, ``note_encoder.note_midi_embed.weight``,
``dur_pred.conv.N.1.weight``, ``diffusion.velocity_fn.*``, ...), so
``load_ckpt(model, work_dir, 'model')`` fills them unchanged.  Everything that builds the
pitch sampler's condition runs in ``pd_pitch_cond_forward``, the sampler in
``pd_reflow_sample`` (``PitchRectifiedFlow``), the whole duration predictor in
``pd_dur_forward`` (include/prodiff_hip.h).  The nn children are parameter containers;
nothing here computes on the CPU and every call raises if the HIP library is unavailable.
"""
from __future__ import annotations

import math

import torch
from torch import nn

from . import _lib
from .prodiff import WaveNet
from .reflow import PitchRectifiedFlow
from .teacher import FastspeechEncoder, SinusoidalPositionalEmbedding, TransformerEncoderLayer


# ---------------------------------------------------------------- parameter containers
class NoteEncoder(nn.Module):
    """tts_modules.py:332-346 (FFTBlocks with use_pos_embed False, use_last_norm; sinusoid positions)."""

    def __init__(self, hidden_size, num_layers, kernel_size, dropout=0.1, num_heads=2):
        super().__init__()
        self.hidden_size, self.num_layers, self.kernel_size, self.num_heads = hidden_size, num_layers, kernel_size, num_heads
        self.layers = nn.ModuleList([TransformerEncoderLayer(hidden_size, kernel_size, num_heads)
                                     for _ in range(num_layers)])
        self.layer_norm = nn.LayerNorm(hidden_size)
        self.note_midi_embed = nn.Linear(1, hidden_size)
        self.note_dur_embed = nn.Linear(1, hidden_size)
        self.embed_scale = math.sqrt(hidden_size)
        self.padding_idx = 0
        self.embed_positions = SinusoidalPositionalEmbedding(hidden_size, 0)

    def ordered_params(self):
        out = []
        for layer in self.layers:
            op = layer.op
            out += [op.layer_norm1.weight, op.layer_norm1.bias, op.self_attn.in_proj_weight,
                    op.self_attn.out_proj.weight, op.layer_norm2.weight, op.layer_norm2.bias,
                    op.ffn.ffn_1.weight, op.ffn.ffn_1.bias, op.ffn.ffn_2.weight, op.ffn.ffn_2.bias]
        return out + [self.layer_norm.weight, self.layer_norm.bias, self.note_midi_embed.weight,
                      self.note_midi_embed.bias, self.note_dur_embed.weight, self.note_dur_embed.bias]


class DurationPredictor(nn.Module):
    """tts_modules.py:59-100: ``conv.i`` is a Sequential with the Conv1d at index 1 and the
    LayerNorm (eps 1e-12, :45) at index 3, as the reference's, so the keys match."""

    def __init__(self, in_dims, n_layers=2, n_chans=384, kernel_size=3, dropout_rate=0.1, offset=1.0,
                 dur_loss_type="mse"):
        super().__init__()
        if dur_loss_type not in ("mse", "huber"):
            raise NotImplementedError(dur_loss_type)
        self.offset, self.kernel_size, self.n_chans, self.loss_type = offset, kernel_size, n_chans, dur_loss_type
        self.conv = nn.ModuleList()
        for idx in range(n_layers):
            self.conv.append(nn.Sequential(
                nn.Identity(),
                nn.Conv1d(in_dims if idx == 0 else n_chans, n_chans, kernel_size, padding=kernel_size // 2),
                nn.ReLU(),
                nn.LayerNorm(n_chans, eps=1e-12),
                nn.Dropout(dropout_rate)))
        self.linear = nn.Linear(n_chans, 1)

    def ordered_params(self):
        out = []
        for seq in self.conv:
            out += [seq[1].weight, seq[1].bias, seq[3].weight, seq[3].bias]
        return out + [self.linear.weight, self.linear.bias]


def _lng(t, dev):
    return None if t is None else t.to(dev).long().reshape(t.shape[0], -1).contiguous()


def _flt(t, dev):
    return None if t is None else t.to(dev).float().reshape(t.shape[0], -1).contiguous()


def _byt(t, dev):
    """bool / integer flags -> one byte each (what the kernels read)."""
    return None if t is None else (t.to(dev) != 0).to(torch.uint8).reshape(t.shape[0], -1).contiguous()


def _vp(t):
    return None if t is None else t.data_ptr()


# ---------------------------------------------------------------- pitch
class PitchPredictor(nn.Module):
    def __init__(self, vocab_size, hparams):
        super().__init__()
        H = hparams["hidden_size"]
        self.vocab_size = vocab_size
        self.encoder = FastspeechEncoder(vocab_size + 1, H, hparams["enc_layers"], hparams["enc_ffn_kernel_size"],
                                         hparams.get("dropout", 0.1), hparams["num_heads"])
        self.with_dur_embed = hparams.get("use_dur_embed", True)
        if not self.with_dur_embed:
            # the reference reads extra_embed unassigned there (pitch_predictor.py:66-70, a NameError at the first call)
            raise ValueError("PitchPredictor needs use_dur_embed=True")
        self.dur_embed = nn.Linear(1, H)
        fa = hparams["f0_prediction_args"]
        ea = fa["encoder_args"]
        self.note_encoder = NoteEncoder(ea["hidden_size"], ea["num_layers"], ea["ffn_kernel_size"],
                                        num_heads=ea["num_heads"])
        self.note_encode_out_linear = nn.Linear(ea["hidden_size"], H)
        self.with_spk_embed = hparams.get("use_spk_id", True)
        if self.with_spk_embed:
            self.spk_embed = nn.Embedding(len(hparams["datasets"]), H)
        self.delta_pitch_embed = nn.Linear(1, H)
        self.pitch_retake_embed = nn.Embedding(2, H)
        da = fa["denoise_args"]
        self.diffusion = PitchRectifiedFlow(
            repeat_bins=fa["repeat_bins"],
            denoise_fn=WaveNet(fa["repeat_bins"], H, da["residual_layers"], da["residual_channels"],
                               da["dilation_cycle_length"]),
            time_scale=fa["timescale"], sampling_algorithm=hparams["sampling_algorithm"],
            spec_min=fa["spec_min"], spec_max=fa["spec_max"], clamp_min=fa["clamp_min"], clamp_max=fa["clamp_max"])
        self._native = _lib.NativeHandle("PitchPredictor", "pd_pitch_cond_create", "pd_pitch_cond_destroy",
                                         num_params="pd_pitch_cond_num_params")
        self._ws = _lib.Workspace()

    def set_compute_dtype(self, dtype):
        """'fp32' (the parity path) or 'bf16' (bf16 MFMA GEMMs, fp32 accumulate) for the condition
        stage and the sampler."""
        self._native.set_dtype(dtype)
        self.diffusion.set_compute_dtype(dtype)
        return self

    # ----------------------------------------------------------- packing
    def cond_dims(self):
        e, n = self.encoder, self.note_encoder
        return _lib.pd_pitch_cond_dims(self.vocab_size, e.hidden_size, e.num_layers, e.kernel_size, e.num_heads,
                                       n.hidden_size, n.num_layers, n.kernel_size, n.num_heads,
                                       self.spk_embed.num_embeddings if self.with_spk_embed else 0,
                                       int(self.with_spk_embed))

    def ordered_cond_params(self):
        """Tensors in the include/prodiff_hip.h pd_pitch_cond order (== reference state-dict order)."""
        out = self.encoder.ordered_params() + [self.dur_embed.weight, self.dur_embed.bias]
        out += self.note_encoder.ordered_params()
        out += [self.note_encode_out_linear.weight, self.note_encode_out_linear.bias]
        if self.with_spk_embed:
            out.append(self.spk_embed.weight)
        return out + [self.delta_pitch_embed.weight, self.delta_pitch_embed.bias, self.pitch_retake_embed.weight]

    def cond_handle(self):
        ps = self.ordered_cond_params()
        return self._native.get(self._native.signature(ps),
                                lambda: (self.cond_dims(), [p.detach().float().contiguous() for p in ps]))

    # ----------------------------------------------------------- forward
    @torch.no_grad()
    def forward_condition(self, txt_tokens, mel2ph, note_midi, note_rest, mel2note, base_pitch, pitch=None,
                          pitch_retake=None, pitch_expr=None, spk_id=None, *, txt_lens=None, note_lens=None):
        """pitch_predictor.py:65-114 -> the sampler's condition [B, T_mel, H] (not in the reference, which
        goes straight on to the diffusion).  ``txt_lens`` / ``note_lens``: each row's phoneme / note count in
        a padded batch -- every row then equals the segment encoded alone (pd_pitch_cond_inputs)."""
        if self.with_spk_embed and spk_id is None:
            raise AssertionError("use_spk_id is True, spk_id is required")
        if pitch_retake is not None and (pitch is None or base_pitch is None):
            raise AssertionError("pitch_retake needs pitch and base_pitch")
        h = self.cond_handle()
        dev = txt_tokens.device
        B, Tt = txt_tokens.shape
        Tn, Tm = note_midi.shape[1], mel2ph.shape[1]
        H = self.encoder.hidden_size
        tok, m2p, m2n = _lng(txt_tokens, dev), _lng(mel2ph, dev), _lng(mel2note, dev)
        midi, rest = _flt(note_midi, dev), _byt(note_rest, dev)
        spk = None if spk_id is None or not self.with_spk_embed else spk_id.to(dev).long().reshape(B).contiguous()
        expr = None if pitch_expr is None else pitch_expr.to(dev).float().reshape(B).contiguous()
        rtk = _byt(pitch_retake, dev)
        pit, base = (_flt(pitch, dev), _flt(base_pitch, dev)) if rtk is not None else (None, None)
        tl = _lib.lens(txt_lens, B, Tt, dev)
        nl = _lib.lens(note_lens, B, Tn, dev)
        keep = (tok, m2p, m2n, midi, rest, spk, expr, rtk, pit, base, tl, nl)
        ins = _lib.pd_pitch_cond_inputs(_vp(tok), _vp(m2p), _vp(midi), _vp(rest), _vp(m2n), _vp(spk), _vp(expr),
                                        _vp(pit), _vp(base), _vp(rtk), _vp(tl), _vp(nl))
        cond = torch.empty(B, Tm, H, device=dev, dtype=torch.float32)
        L = _lib.lib()
        ws, wsb = self._ws.get(L.pd_pitch_cond_workspace_size(h, B, Tt, Tn, Tm), dev)
        _lib.check(L.pd_pitch_cond_forward(h, _lib.C.byref(ins), _lib.fptr(cond), B, Tt, Tn, Tm, ws, wsb,
                                           _lib.stream_ptr(dev)))
        del keep
        return cond

    def forward(self, txt_tokens, mel2ph, note_midi, note_rest, mel2note, base_pitch, pitch=None, pitch_retake=None,
                pitch_expr=None, spk_id=None, infer_step=20, infer=False):
        """pitch_predictor.py:57-121 (inference only) -> delta pitch [B, T_mel]."""
        if not infer:
            raise NotImplementedError("training (infer=False) is out of scope")
        condition = self.forward_condition(txt_tokens, mel2ph, note_midi, note_rest, mel2note, base_pitch,
                                           pitch=pitch, pitch_retake=pitch_retake, pitch_expr=pitch_expr,
                                           spk_id=spk_id)
        return self.diffusion(condition, infer_step=infer_step, infer=True)


# ---------------------------------------------------------------- duration
class DurPredictor(nn.Module):
    def __init__(self, vocab_size, hparams):
        super().__init__()
        H = hparams["hidden_size"]
        self.vocab_size = vocab_size
        self.encoder = FastspeechEncoder(vocab_size, H, hparams["enc_layers"], hparams["enc_ffn_kernel_size"],
                                         num_heads=hparams["num_heads"])
        dh = hparams["dur_prediction_args"]
        self.onset_embed = nn.Embedding(2, H)
        self.word_dur_embed = nn.Linear(1, H)
        self.dur_pred = DurationPredictor(H, n_layers=dh["num_layers"], n_chans=dh["hidden_size"],
                                          dropout_rate=dh["dropout"], kernel_size=dh["kernel_size"],
                                          offset=dh["log_offset"], dur_loss_type=dh["loss_type"])
        self._native = _lib.NativeHandle("DurPredictor", "pd_dur_create", "pd_dur_destroy",
                                         num_params="pd_dur_num_params")
        self._ws = _lib.Workspace()

    def set_compute_dtype(self, dtype):
        """'fp32' (the parity path) or 'bf16' (bf16 MFMA GEMMs, fp32 accumulate)."""
        self._native.set_dtype(dtype)
        return self

    def dur_dims(self):
        e, p = self.encoder, self.dur_pred
        return _lib.pd_dur_dims(self.vocab_size, e.hidden_size, e.num_layers, e.kernel_size, e.num_heads,
                                len(p.conv), p.n_chans, p.kernel_size, float(p.offset))

    def ordered_dur_params(self):
        """Tensors in the include/prodiff_hip.h pd_dur order (== reference state-dict order)."""
        return (self.encoder.ordered_params() + [self.onset_embed.weight, self.word_dur_embed.weight,
                                                 self.word_dur_embed.bias] + self.dur_pred.ordered_params())

    def dur_handle(self):
        ps = self.ordered_dur_params()
        return self._native.get(self._native.signature(ps, float(self.dur_pred.offset)),
                                lambda: (self.dur_dims(), [p.detach().float().contiguous() for p in ps]))

    @torch.no_grad()
    def forward(self, txt_tokens, onset, word_dur, infer=True, *, return_log=False, txt_lens=None):
        """dur_predictor.py:31-36 -> phoneme durations [B, T_txt] (clamped at 0 when ``infer``).
        ``return_log`` (not in the reference) also returns the log-domain prediction, the masked output of
        ``dur_pred.linear``; ``txt_lens`` as ProDiffTeacher.forward_condition's."""
        if not infer:
            raise NotImplementedError("training (infer=False: unclamped durations) is out of scope")
        h = self.dur_handle()
        dev = txt_tokens.device
        B, Tt = txt_tokens.shape
        tok, ons, wd = _lng(txt_tokens, dev), _lng(onset, dev), _flt(word_dur, dev)
        tl = _lib.lens(txt_lens, B, Tt, dev)
        keep = (tok, ons, wd, tl)
        ins = _lib.pd_dur_inputs(_vp(tok), _vp(ons), _vp(wd), _vp(tl))
        log = torch.empty(B, Tt, device=dev, dtype=torch.float32)
        dur = torch.empty(B, Tt, device=dev, dtype=torch.float32)
        L = _lib.lib()
        ws, wsb = self._ws.get(L.pd_dur_workspace_size(h, B, Tt), dev)
        _lib.check(L.pd_dur_forward(h, _lib.C.byref(ins), _lib.fptr(log), _lib.fptr(dur), B, Tt, ws, wsb,
                                    _lib.stream_ptr(dev)))
        del keep
        return (dur, log) if return_log else dur
