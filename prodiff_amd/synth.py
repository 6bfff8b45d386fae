"""Seeded synthetic parameters and inputs shared by the golden-vector script,
the parity tests and ``bench.py``.

No pretrained checkpoint exists offline, so every parity
fixture is produced with weights drawn here.  The draw is keyed by
``(seed, crc32(parameter name))`` with numpy's PCG64 generator, which is
bit-stable across machines, so the GPU box regenerates exactly the weights the
reference saw in this container without any weight file travelling.

Parameter names and shapes follow the reference state dicts:
  * ``WaveNet``  -- modules/decoder/wavenet.py:74-99
  * ``FastDiff`` -- modules/FastDiff/module/FastDiff_model.py:13-72 (weight-norm
    form, ``weight_g``/``weight_v``, as the checkpoints store it:
    component/vocoder/fastdiff.py:41)
"""
from __future__ import annotations

import zlib
from collections import OrderedDict

import numpy as np


# --------------------------------------------------------------------------
# parameter name/shape tables
# --------------------------------------------------------------------------
def wavenet_param_shapes(in_dims=80, hidden_size=256, residual_layers=20,
                         residual_channels=256):
    """Ordered ``{state-dict key: shape}`` of reference ``WaveNet``."""
    C, H, M = residual_channels, hidden_size, in_dims
    s = OrderedDict()
    s["input_projection.weight"] = (C, M, 1)
    s["input_projection.bias"] = (C,)
    s["mlp.0.weight"] = (4 * C, C)
    s["mlp.0.bias"] = (4 * C,)
    s["mlp.2.weight"] = (C, 4 * C)
    s["mlp.2.bias"] = (C,)
    for l in range(residual_layers):
        p = f"residual_layers.{l}."
        s[p + "dilated_conv.weight"] = (2 * C, C, 3)
        s[p + "dilated_conv.bias"] = (2 * C,)
        s[p + "diffusion_projection.weight"] = (C, C)
        s[p + "diffusion_projection.bias"] = (C,)
        s[p + "conditioner_projection.weight"] = (2 * C, H, 1)
        s[p + "conditioner_projection.bias"] = (2 * C,)
        s[p + "output_projection.weight"] = (2 * C, C, 1)
        s[p + "output_projection.bias"] = (2 * C,)
    s["skip_projection.weight"] = (C, C, 1)
    s["skip_projection.bias"] = (C,)
    s["output_projection.weight"] = (M, C, 1)
    s["output_projection.bias"] = (M,)
    return s


KPNET_RES_IDX = (1, 3, 6, 8, 11, 13)   # Conv1d positions inside residual_conv (modules.py:297-313)


def _wn(s, name, shape):
    s[name + ".bias"] = (shape[0],)
    s[name + ".weight_g"] = (shape[0], 1, 1)
    s[name + ".weight_v"] = tuple(shape)


def fastdiff_param_shapes(audio_channels=1, inner_channels=32, cond_channels=80,
                          upsample_ratios=(8, 8, 4), lvc_layers_each_block=4,
                          lvc_kernel_size=3, kpnet_hidden_channels=64,
                          kpnet_conv_size=3, diffusion_step_embed_dim_in=128,
                          diffusion_step_embed_dim_mid=512,
                          diffusion_step_embed_dim_out=512, weight_norm=True):
    """Ordered ``{state-dict key: shape}`` of reference ``FastDiff``.

    With ``weight_norm`` every ``nn.Conv1d`` carries ``weight_g``/``weight_v``
    (FastDiff_model.py:115-122); ``ConvTranspose1d`` and ``Linear`` do not.
    """
    Ci, Cc, Hk = inner_channels, cond_channels, kpnet_hidden_channels
    Lyr, ks, kp = lvc_layers_each_block, lvc_kernel_size, kpnet_conv_size
    s = OrderedDict()

    def conv(name, shape):
        if weight_norm:
            _wn(s, name, shape)
        else:
            s[name + ".weight"] = tuple(shape)
            s[name + ".bias"] = (shape[0],)

    conv("first_audio_conv", (Ci, audio_channels, 7))
    s["fc_t1.weight"] = (diffusion_step_embed_dim_mid, diffusion_step_embed_dim_in)
    s["fc_t1.bias"] = (diffusion_step_embed_dim_mid,)
    s["fc_t2.weight"] = (diffusion_step_embed_dim_out, diffusion_step_embed_dim_mid)
    s["fc_t2.bias"] = (diffusion_step_embed_dim_out,)
    nb = len(upsample_ratios)
    for n in range(nb):
        r = upsample_ratios[n]
        p = f"lvc_blocks.{n}."
        s[p + "upsample.weight"] = (Ci, Ci, 2 * r)
        s[p + "upsample.bias"] = (Ci,)
        conv(p + "kernel_predictor.input_conv.0", (Hk, Cc, 5))
        for j in KPNET_RES_IDX:
            conv(p + f"kernel_predictor.residual_conv.{j}", (Hk, Hk, kp))
        conv(p + "kernel_predictor.kernel_conv", (Ci * 2 * Ci * ks * Lyr, Hk, kp))
        conv(p + "kernel_predictor.bias_conv", (2 * Ci * Lyr, Hk, kp))
        s[p + "fc_t.weight"] = (Cc, diffusion_step_embed_dim_out)
        s[p + "fc_t.bias"] = (Cc,)
        for i in range(Lyr):
            conv(p + f"convs.{i}", (Ci, Ci, ks))
    for n in range(nb):
        p = f"downsample.{n}."
        conv(p + "residual_dense", (Ci, Ci, 1))
        for j in range(3):
            conv(p + f"conv.{j}", (Ci, Ci, 3))
    conv("final_conv.0", (audio_channels, Ci, 7))
    return s


# --------------------------------------------------------------------------
# draws
# --------------------------------------------------------------------------
def _rng(seed, name):
    return np.random.default_rng([int(seed), zlib.crc32(name.encode())])


def _gain(name):
    # the LVC kernels multiply 96 taps each; keep them from saturating the gate
    if "kernel_conv" in name or "bias_conv" in name:
        return 0.3
    # a trained eps-network predicts ~N(0,1); keep the synthetic one there too
    if "final_conv" in name:
        return 0.2
    # NSF-HiFiGAN output conv feeds a tanh: keep it out of saturation
    if name.startswith("conv_post"):
        return 0.3
    # durations reach tens of frames; keep dur * w at the embedding scale
    if name.startswith("dur_embed"):
        return 0.1
    return 1.0


def synth_tensor(name, shape, seed):
    """Deterministic float32 draw for one parameter."""
    rng = _rng(seed, name)
    z = rng.standard_normal(size=shape, dtype=np.float32)
    if name.endswith(".bias"):
        return (0.02 * z).astype(np.float32)
    if name.endswith(".weight_g"):
        return (_gain(name) * (1.0 + 0.1 * z)).astype(np.float32)
    if name.endswith(".weight_v"):
        return z
    if "layer_norm" in name and name.endswith(".weight"):   # LayerNorm gamma ~ 1
        return (1.0 + 0.1 * z).astype(np.float32)
    if "upsample" in name or name.startswith("ups."):   # ConvTranspose1d [Cin, Cout, k]: 2 taps hit each output
        fan_in = shape[0] * 2
    else:
        fan_in = int(np.prod(shape[1:]))
    return (z * (_gain(name) / np.sqrt(fan_in))).astype(np.float32)


def synth_params(shapes, seed):
    return OrderedDict((k, synth_tensor(k, v, seed)) for k, v in shapes.items())


def fold_weight_norm_np(g, v):
    """w = g * v / ||v|| with the norm over every dim but 0 (torch.nn.utils.weight_norm, dim=0)."""
    n = np.sqrt(np.sum(v.astype(np.float64) ** 2, axis=tuple(range(1, v.ndim)), keepdims=True))
    return (g.astype(np.float64) * v / n).astype(np.float32)


def synth_inputs(seed, shape, kind="normal", loc=0.0, scale=1.0):
    rng = np.random.default_rng([int(seed), 0xC0FFEE])
    if kind == "uniform":
        return rng.random(size=shape, dtype=np.float32)
    return (loc + scale * rng.standard_normal(size=shape, dtype=np.float32)).astype(np.float32)


# NSF-HiFiGAN generator (modules/nsf_hifigan/models.py:208-265), plain (weight-norm
# removed) keys in state-dict order.  Default dims are the SVS vocoder's
# (handler/base_config.yaml:7-11: 128 mels, 44.1 kHz, hop 512 = 8*8*2*2*2).
NSF_DEFAULTS = dict(num_mels=128, upsample_initial_channel=512, upsample_rates=(8, 8, 2, 2, 2),
                    upsample_kernel_sizes=(16, 16, 4, 4, 4), resblock="1", resblock_kernel_sizes=(3, 7, 11),
                    resblock_dilation_sizes=((1, 3, 5), (1, 3, 5), (1, 3, 5)), sampling_rate=44100)


def nsf_param_shapes(num_mels=128, upsample_initial_channel=512, upsample_rates=(8, 8, 2, 2, 2),
                     upsample_kernel_sizes=(16, 16, 4, 4, 4), resblock="1", resblock_kernel_sizes=(3, 7, 11),
                     resblock_dilation_sizes=((1, 3, 5), (1, 3, 5), (1, 3, 5)), harmonic_num=8, **_):
    s = OrderedDict()
    s["m_source.l_linear.weight"] = (1, harmonic_num + 1)
    s["m_source.l_linear.bias"] = (1,)
    ch0 = upsample_initial_channel
    for i in range(len(upsample_rates)):
        c = ch0 // 2 ** (i + 1)
        if i + 1 < len(upsample_rates):
            sf = int(np.prod(upsample_rates[i + 1:]))
            s[f"noise_convs.{i}.weight"] = (c, 1, 2 * sf)
        else:
            s[f"noise_convs.{i}.weight"] = (c, 1, 1)
        s[f"noise_convs.{i}.bias"] = (c,)
    s["conv_pre.weight"] = (ch0, num_mels, 7)
    s["conv_pre.bias"] = (ch0,)
    for i, (u, k) in enumerate(zip(upsample_rates, upsample_kernel_sizes)):
        s[f"ups.{i}.weight"] = (ch0 // 2 ** i, ch0 // 2 ** (i + 1), k)
        s[f"ups.{i}.bias"] = (ch0 // 2 ** (i + 1),)
    n = 0
    for i in range(len(upsample_rates)):
        c = ch0 // 2 ** (i + 1)
        for k, d in zip(resblock_kernel_sizes, resblock_dilation_sizes):
            names = ([f"convs1.{j}" for j in range(len(d))] + [f"convs2.{j}" for j in range(len(d))]
                     if str(resblock) == "1" else [f"convs.{j}" for j in range(len(d))])
            for nm in names:
                s[f"resblocks.{n}.{nm}.weight"] = (c, c, k)
                s[f"resblocks.{n}.{nm}.bias"] = (c,)
            n += 1
    s["conv_post.weight"] = (1, ch0 // 2 ** len(upsample_rates), 7)
    s["conv_post.bias"] = (1,)
    return s


# --------------------------------------------------------------------------
# SVS teacher condition stage (modules/svs/prodiff_teacher.py:10-47, encoder
# modules/fastspeech/tts_modules.py:291-308, layers common_layers.py:625-648)
# --------------------------------------------------------------------------
COND_DEFAULTS = dict(hidden_size=256, enc_layers=4, enc_ffn_kernel_size=9, num_heads=2, num_spk=1, num_langs=3,
                     use_dur_embed=True, use_spk_id=True, use_gender_id=False, use_lang_id=True,
                     use_voicing_embed=True, use_breath_embed=True)


def cond_param_shapes(vocab_size, hidden_size=256, enc_layers=4, enc_ffn_kernel_size=9, num_spk=1, num_langs=3,
                      use_dur_embed=True, use_spk_id=True, use_gender_id=False, use_lang_id=True,
                      use_voicing_embed=True, use_breath_embed=True, **_):
    """Ordered ``{state-dict key: shape}`` of the teacher minus ``diffusion.*`` and buffers."""
    H, k = hidden_size, enc_ffn_kernel_size
    s = OrderedDict()
    for l in range(enc_layers):
        p = f"encoder.layers.{l}.op."
        s[p + "layer_norm1.weight"] = (H,)
        s[p + "layer_norm1.bias"] = (H,)
        s[p + "self_attn.in_proj_weight"] = (3 * H, H)
        s[p + "self_attn.out_proj.weight"] = (H, H)
        s[p + "layer_norm2.weight"] = (H,)
        s[p + "layer_norm2.bias"] = (H,)
        s[p + "ffn.ffn_1.weight"] = (4 * H, H, k)
        s[p + "ffn.ffn_1.bias"] = (4 * H,)
        s[p + "ffn.ffn_2.weight"] = (H, 4 * H)
        s[p + "ffn.ffn_2.bias"] = (H,)
    s["encoder.layer_norm.weight"] = (H,)
    s["encoder.layer_norm.bias"] = (H,)
    s["encoder.embed_tokens.weight"] = (vocab_size, H)
    if use_dur_embed:
        s["dur_embed.weight"] = (H, 1)
        s["dur_embed.bias"] = (H,)
    if use_spk_id:
        s["spk_embed.weight"] = (num_spk, H)
    if use_gender_id:
        s["gender_embed.weight"] = (2, H)
    if use_lang_id:
        s["lang_embed.weight"] = (num_langs, H)
    s["pitch_embed.weight"] = (H, 1)
    s["pitch_embed.bias"] = (H,)
    if use_voicing_embed:
        s["voicing_embed.weight"] = (H, 1)
        s["voicing_embed.bias"] = (H,)
    if use_breath_embed:
        s["breath_embed.weight"] = (H, 1)
        s["breath_embed.bias"] = (H,)
    return s


def synth_cond_params(shapes, seed):
    """synth_params + the padding rows Embedding(..., padding_idx=0) keeps at zero
    (common_layers.py:63-68: initialised to 0 and never updated)."""
    P = synth_params(shapes, seed)
    for k in ("encoder.embed_tokens.weight", "lang_embed.weight"):
        if k in P:
            P[k][0] = 0.0
    return P


def synth_cond_inputs(seed, lengths, vocab_size, num_spk=1, num_langs=3, max_dur=12, pad_tokens=0):
    """Ragged batch of phoneme sequences with durations: ``lengths[b]`` tokens (ids >= 1) then
    zero padding to max(lengths) + pad_tokens; mel2ph repeats token i+1 dur[i] times, then
    0-padding to the longest utterance (the binarizer's layout, tts_modules.py:135-171)."""
    rng = np.random.default_rng([int(seed), 0xC0D])
    B = len(lengths)
    Tt = max(lengths) + pad_tokens
    tok = np.zeros((B, Tt), np.int64)
    lang = np.zeros((B, Tt), np.int64)
    durs = []
    for b, n in enumerate(lengths):
        tok[b, :n] = rng.integers(1, vocab_size, n)
        lang[b, :n] = rng.integers(1, max(num_langs, 2), n)
        durs.append(rng.integers(1, max_dur + 1, n))
    Tm = max(int(d.sum()) for d in durs)
    mel2ph = np.zeros((B, Tm), np.int64)
    for b, d in enumerate(durs):
        mel2ph[b, :int(d.sum())] = np.repeat(np.arange(1, len(d) + 1), d)
    f0 = rng.uniform(80.0, 800.0, (B, Tm)).astype(np.float32)
    f0[rng.random((B, Tm)) < 0.15] = 0.0        # unvoiced frames
    voicing = rng.uniform(-1.5, 1.0, (B, Tm)).astype(np.float32)
    breath = rng.uniform(-1.5, 1.0, (B, Tm)).astype(np.float32)
    spk = rng.integers(0, num_spk, B).astype(np.int64)
    return dict(txt_tokens=tok, mel2ph=mel2ph, f0=f0, lang_seq=lang, spk_embed_id=spk,
                voicing=voicing, breath=breath)


def synth_svs_utterance(seed, frames, n_tokens, vocab_size, num_langs=3, hidden=256):
    """One SVS segment as the inference handler builds it (handler/infer/handler.py:220-262):
    n_tokens phonemes whose durations sum to exactly `frames` mel frames, f0 with unvoiced
    gaps, voicing / breath curves and a time-invariant speaker mix [1, H]."""
    rng = np.random.default_rng([int(seed), 0x5F5])
    cuts = np.sort(rng.choice(np.arange(1, frames), n_tokens - 1, replace=False))
    dur = np.diff(np.concatenate([[0], cuts, [frames]]))
    tok = rng.integers(1, vocab_size, n_tokens).astype(np.int64)
    lang = rng.integers(1, max(num_langs, 2), n_tokens).astype(np.int64)
    mel2ph = np.repeat(np.arange(1, n_tokens + 1), dur).astype(np.int64)
    f0 = rng.uniform(120.0, 700.0, frames).astype(np.float32)
    f0[rng.random(frames) < 0.1] = 0.0
    return dict(txt_tokens=tok, mel2ph=mel2ph, f0=f0, lang_seq=lang,
                spk_mix_embed=(0.3 * rng.standard_normal((1, hidden))).astype(np.float32),
                voicing=rng.uniform(-1.5, 1.0, frames).astype(np.float32),
                breath=rng.uniform(-1.5, 1.0, frames).astype(np.float32))


# --------------------------------------------------------------------------
# Variance predictors (modules/variance_predictor/{pitch,dur}_predictor.py; encoders
# modules/fastspeech/tts_modules.py:291-365, DurationPredictor :59-100)
# --------------------------------------------------------------------------
PITCH_DEFAULTS = dict(hidden_size=256, enc_layers=4, enc_ffn_kernel_size=9, num_heads=2, note_hidden_size=128,
                      note_layers=4, note_ffn_kernel_size=9, note_heads=2, num_spk=1, use_spk_id=True)
DUR_DEFAULTS = dict(hidden_size=256, enc_layers=4, enc_ffn_kernel_size=9, num_heads=2, n_layers=5, n_chans=512,
                    kernel_size=3, log_offset=1.0)


def _fft_shapes(s, prefix, H, k, layers):
    """FFTBlocks parameters (layers then the final LayerNorm) in state-dict order."""
    for l in range(layers):
        p = f"{prefix}layers.{l}.op."
        s[p + "layer_norm1.weight"] = (H,)
        s[p + "layer_norm1.bias"] = (H,)
        s[p + "self_attn.in_proj_weight"] = (3 * H, H)
        s[p + "self_attn.out_proj.weight"] = (H, H)
        s[p + "layer_norm2.weight"] = (H,)
        s[p + "layer_norm2.bias"] = (H,)
        s[p + "ffn.ffn_1.weight"] = (4 * H, H, k)
        s[p + "ffn.ffn_1.bias"] = (4 * H,)
        s[p + "ffn.ffn_2.weight"] = (H, 4 * H)
        s[p + "ffn.ffn_2.bias"] = (H,)
    s[prefix + "layer_norm.weight"] = (H,)
    s[prefix + "layer_norm.bias"] = (H,)


def pitch_param_shapes(vocab_size, hidden_size=256, enc_layers=4, enc_ffn_kernel_size=9, note_hidden_size=128,
                       note_layers=4, note_ffn_kernel_size=9, num_spk=1, use_spk_id=True, **_):
    """Ordered ``{state-dict key: shape}`` of the reference PitchPredictor minus ``diffusion.*`` and buffers."""
    H, Hn = hidden_size, note_hidden_size
    s = OrderedDict()
    _fft_shapes(s, "encoder.", H, enc_ffn_kernel_size, enc_layers)
    s["encoder.embed_tokens.weight"] = (vocab_size + 1, H)
    s["dur_embed.weight"] = (H, 1)
    s["dur_embed.bias"] = (H,)
    _fft_shapes(s, "note_encoder.", Hn, note_ffn_kernel_size, note_layers)
    s["note_encoder.note_midi_embed.weight"] = (Hn, 1)
    s["note_encoder.note_midi_embed.bias"] = (Hn,)
    s["note_encoder.note_dur_embed.weight"] = (Hn, 1)
    s["note_encoder.note_dur_embed.bias"] = (Hn,)
    s["note_encode_out_linear.weight"] = (H, Hn)
    s["note_encode_out_linear.bias"] = (H,)
    if use_spk_id:
        s["spk_embed.weight"] = (num_spk, H)
    s["delta_pitch_embed.weight"] = (H, 1)
    s["delta_pitch_embed.bias"] = (H,)
    s["pitch_retake_embed.weight"] = (2, H)
    return s


def dur_param_shapes(vocab_size, hidden_size=256, enc_layers=4, enc_ffn_kernel_size=9, n_layers=5, n_chans=512,
                     kernel_size=3, **_):
    """Ordered ``{state-dict key: shape}`` of the reference DurPredictor minus buffers."""
    H, C = hidden_size, n_chans
    s = OrderedDict()
    _fft_shapes(s, "encoder.", H, enc_ffn_kernel_size, enc_layers)
    s["encoder.embed_tokens.weight"] = (vocab_size, H)
    s["onset_embed.weight"] = (2, H)
    s["word_dur_embed.weight"] = (H, 1)
    s["word_dur_embed.bias"] = (H,)
    for i in range(n_layers):
        s[f"dur_pred.conv.{i}.1.weight"] = (C, H if i == 0 else C, kernel_size)
        s[f"dur_pred.conv.{i}.1.bias"] = (C,)
        s[f"dur_pred.conv.{i}.3.weight"] = (C,)
        s[f"dur_pred.conv.{i}.3.bias"] = (C,)
    s["dur_pred.linear.weight"] = (1, C)
    s["dur_pred.linear.bias"] = (1,)
    return s


def synth_variance_params(shapes, seed, dur_bias=None):
    """synth_cond_params (the zero padding row of embed_tokens), the duration predictor's LayerNorm gamma
    near 1 (``conv.i.3.weight``), the note embeddings at the scale of their inputs (MIDI numbers reach 80,
    durations tens of frames) and, for the duration fixtures, a chosen ``dur_pred.linear.bias``: synthetic
    weights otherwise put exp(log) - 1 below 0 on almost every token and the clamp hides the head."""
    P = synth_cond_params(shapes, seed)
    for k in P:
        if k.startswith("dur_pred.conv.") and k.endswith(".3.weight"):
            P[k] = (1.0 + 0.1 * _rng(seed, k).standard_normal(size=P[k].shape, dtype=np.float32)).astype(np.float32)
        if k in ("note_encoder.note_midi_embed.weight", "note_encoder.note_dur_embed.weight"):
            P[k] = (P[k] * np.float32(0.02)).astype(np.float32)
    if dur_bias is not None:
        P["dur_pred.linear.bias"] = np.full((1,), dur_bias, np.float32)
    return P


def _spans(rng, counts, max_dur, Tm=None):
    """mel2x rows: item i+1 repeated dur[i] times, 0-padded to the longest row (or Tm)."""
    durs = [rng.integers(1, max_dur + 1, n) for n in counts]
    Tm = Tm or max(int(d.sum()) for d in durs)
    out = np.zeros((len(counts), Tm), np.int64)
    for b, d in enumerate(durs):
        seq = np.repeat(np.arange(1, len(d) + 1), d)[:Tm]
        out[b, :len(seq)] = seq
    return out


def synth_pitch_inputs(seed, lengths, note_lengths, vocab_size, num_spk=1, pad_tokens=0, pad_notes=0, frames=None,
                       retake=False, max_dur=6):
    """PitchPredictor.forward's inputs for a ragged batch: ``lengths[b]`` phonemes (ids in [1, vocab_size])
    and ``note_lengths[b]`` notes (MIDI 48..76, about a fifth of them rests) per row, padded with token 0 /
    midi -1; mel2ph and mel2note cover the same frames of a row (the first ``frames``, or the row's phoneme
    durations) and are 0 after them.  ``retake``: pitch, pitch_retake (about half the frames) instead of
    pitch_expr (one value per row)."""
    rng = np.random.default_rng([int(seed), 0x917C])
    B = len(lengths)
    Tt, Tn = max(lengths) + pad_tokens, max(note_lengths) + pad_notes
    tok = np.zeros((B, Tt), np.int64)
    midi = np.full((B, Tn), -1.0, np.float32)
    rest = np.zeros((B, Tn), bool)
    for b, (n, m) in enumerate(zip(lengths, note_lengths)):
        tok[b, :n] = rng.integers(1, vocab_size + 1, n)
        midi[b, :m] = rng.integers(48, 77, m).astype(np.float32) + rng.integers(0, 2, m) * np.float32(0.5)
        rest[b, :m] = rng.random(m) < 0.2
    if frames is None:
        mel2ph = _spans(rng, lengths, max_dur)
    else:
        mel2ph = np.zeros((B, frames), np.int64)
        for b, n in enumerate(lengths):
            cuts = np.sort(rng.choice(np.arange(1, frames), n - 1, replace=False))
            mel2ph[b] = np.repeat(np.arange(1, n + 1), np.diff(np.concatenate([[0], cuts, [frames]])))
    Tm = mel2ph.shape[1]
    mel2note = np.zeros((B, Tm), np.int64)
    for b, m in enumerate(note_lengths):
        nf = int((mel2ph[b] > 0).sum())
        cuts = np.sort(rng.choice(np.arange(1, nf), m - 1, replace=False))
        mel2note[b, :nf] = np.repeat(np.arange(1, m + 1), np.diff(np.concatenate([[0], cuts, [nf]])))
    base = np.take_along_axis(np.concatenate([np.full((B, 1), -1.0, np.float32), midi], 1), mel2note, 1)
    x = dict(txt_tokens=tok, mel2ph=mel2ph, note_midi=midi, note_rest=rest, mel2note=mel2note,
             base_pitch=base.astype(np.float32), spk_id=rng.integers(0, num_spk, B).astype(np.int64))
    if retake:
        x["pitch"] = (base + rng.uniform(-1.5, 1.5, (B, Tm))).astype(np.float32)
        x["pitch_retake"] = rng.random((B, Tm)) < 0.5
    else:
        x["pitch_expr"] = rng.uniform(0.0, 1.0, (B, 1)).astype(np.float32)
    return x


def synth_dur_inputs(seed, lengths, vocab_size, pad_tokens=0):
    """DurPredictor.forward's inputs: ``lengths[b]`` phonemes (ids in [1, vocab_size)) then token 0; onset 1
    on the first phoneme of a word (about every third), word_dur the word's length in seconds on each of its
    phonemes (handler/infer/handler.py:219-227), 0 on padding."""
    rng = np.random.default_rng([int(seed), 0xD0B])
    B, Tt = len(lengths), max(lengths) + pad_tokens
    tok = np.zeros((B, Tt), np.int64)
    onset = np.zeros((B, Tt), np.int64)
    wd = np.zeros((B, Tt), np.float32)
    for b, n in enumerate(lengths):
        tok[b, :n] = rng.integers(1, vocab_size, n)
        on = (rng.random(n) < 0.35).astype(np.int64)
        on[0] = 1
        onset[b, :n] = on
        word = np.cumsum(on) - 1
        wd[b, :n] = rng.uniform(0.1, 1.2, int(word.max()) + 1).astype(np.float32)[word]
    return dict(txt_tokens=tok, onset=onset, word_dur=wd)


# --------------------------------------------------------------------------
# RMVPE pitch extractor (modules/rmvpe/model.py E2E0): state-dict order without the
# num_batches_tracked counters and without unet.tf.* (built, never called)
# --------------------------------------------------------------------------
RMVPE_DEFAULTS = dict(n_blocks=4, n_gru=1, en_de_layers=5, inter_layers=4, en_out_channels=16)
RMVPE_N_MELS, RMVPE_N_CLASS, RMVPE_GRU_HIDDEN = 128, 360, 256
RMVPE_FC_GAIN = 2.0        # the final Linear: spreads the salience over (0.01, 0.97) without saturating it
# the convs: about a hundred residual blocks add their ReLU outputs up with no normalisation of the sum; at
# gain 1 the full model's features reach 3e3 and its salience saturates (torch's own default init is 1/sqrt(3))
RMVPE_CONV_GAIN = 0.5
RMVPE_SKIPPED = ("unet.tf.", "num_batches_tracked")


def rmvpe_key_is_skipped(key):
    return key.startswith(RMVPE_SKIPPED[0]) or key.endswith(RMVPE_SKIPPED[1])


def _rmvpe_bn(s, p, C):
    for leaf in ("weight", "bias", "running_mean", "running_var"):
        s[f"{p}.{leaf}"] = (C,)


def _rmvpe_block(s, p, cin, cout):
    s[p + ".conv.0.weight"] = (cout, cin, 3, 3)
    _rmvpe_bn(s, p + ".conv.1", cout)
    s[p + ".conv.3.weight"] = (cout, cout, 3, 3)
    _rmvpe_bn(s, p + ".conv.4", cout)
    if cin != cout:
        s[p + ".shortcut.weight"] = (cout, cin, 1, 1)
        s[p + ".shortcut.bias"] = (cout,)


def rmvpe_param_shapes(n_blocks=4, n_gru=1, en_de_layers=5, inter_layers=4, en_out_channels=16,
                       n_mels=RMVPE_N_MELS, n_class=RMVPE_N_CLASS, gru_hidden=RMVPE_GRU_HIDDEN):
    """Ordered ``{key: shape}`` of the parameters pd_rmvpe_create takes (include/prodiff_hip.h)."""
    L, c0, s = en_de_layers, en_out_channels, OrderedDict()
    _rmvpe_bn(s, "unet.encoder.bn", 1)
    for i in range(L):
        cin, cout = (1 if i == 0 else c0 << (i - 1)), c0 << i
        for j in range(n_blocks):
            _rmvpe_block(s, f"unet.encoder.layers.{i}.conv.{j}", cin if j == 0 else cout, cout)
    for i in range(inter_layers):
        cin, cout = (c0 << (L - 1) if i == 0 else c0 << L), c0 << L
        for j in range(n_blocks):
            _rmvpe_block(s, f"unet.intermediate.layers.{i}.conv.{j}", cin if j == 0 else cout, cout)
    for i in range(L):
        cout = c0 << (L - 1 - i)
        s[f"unet.decoder.layers.{i}.conv1.0.weight"] = (2 * cout, cout, 3, 3)
        _rmvpe_bn(s, f"unet.decoder.layers.{i}.conv1.1", cout)
        for j in range(n_blocks):
            _rmvpe_block(s, f"unet.decoder.layers.{i}.conv2.{j}", 2 * cout if j == 0 else cout, cout)
    s["cnn.weight"] = (3, c0, 3, 3)
    s["cnn.bias"] = (3,)
    if n_gru:
        for suffix in ("", "_reverse"):
            s["fc.0.gru.weight_ih_l0" + suffix] = (3 * gru_hidden, 3 * n_mels)
            s["fc.0.gru.weight_hh_l0" + suffix] = (3 * gru_hidden, gru_hidden)
            s["fc.0.gru.bias_ih_l0" + suffix] = (3 * gru_hidden,)
            s["fc.0.gru.bias_hh_l0" + suffix] = (3 * gru_hidden,)
        s["fc.1.weight"] = (n_class, 2 * gru_hidden)
        s["fc.1.bias"] = (n_class,)
    else:
        s["fc.0.weight"] = (n_class, 3 * n_mels)
        s["fc.0.bias"] = (n_class,)
    return s


def synth_rmvpe_tensor(name, shape, seed, fc_gain=RMVPE_FC_GAIN):
    """The RMVPE draw rules: conv / GRU / Linear weights by fan-in (ConvTranspose2d [Cin, Cout, 3, 3]: at most
    four taps of each input channel reach an output), BatchNorm gamma and running_var uniform in [0.75, 1.25],
    BatchNorm beta and running_mean 0.1 N(0, 1), other biases 0.02 N(0, 1), the final Linear times ``fc_gain``."""
    rng = _rng(seed, name)
    leaf = name.rsplit(".", 1)[-1]
    is_bn = _rmvpe_is_bn(name)
    if is_bn and leaf in ("weight", "running_var"):
        return (0.75 + 0.5 * rng.random(size=shape, dtype=np.float32)).astype(np.float32)
    z = rng.standard_normal(size=shape, dtype=np.float32)
    if is_bn:
        return (0.1 * z).astype(np.float32)
    if len(shape) == 1:
        return (0.02 * z).astype(np.float32)
    if ".conv1.0." in name:
        fan_in = shape[0] * 4
    else:
        fan_in = int(np.prod(shape[1:]))
    gain = fc_gain if name in ("fc.1.weight", "fc.0.weight") else (RMVPE_CONV_GAIN if len(shape) == 4 else 1.0)
    return (z * (gain / np.sqrt(fan_in))).astype(np.float32)


def _rmvpe_is_bn(name):
    """The BatchNorms are the children 1 and 4 of a block's conv stack, child 1 of a decoder level's conv1
    and the encoder's input norm."""
    return name.rsplit(".", 1)[0].endswith((".conv.1", ".conv.4", ".conv1.1", "encoder.bn"))


def synth_rmvpe_params(shapes, seed, fc_gain=RMVPE_FC_GAIN):
    return OrderedDict((k, synth_rmvpe_tensor(k, v, seed, fc_gain)) for k, v in shapes.items())


# --------------------------------------------------------------------------
# Harmonic-noise separation (modules/vr/nets.py CascadedNet, is_complex = True): state-dict order without the
# num_batches_tracked counters
# --------------------------------------------------------------------------
def _vr_cba(s, p, cin, cout, k):
    s[p + ".conv.0.weight"] = (cout, cin, k, k)
    for leaf in ("weight", "bias", "running_mean", "running_var"):
        s[f"{p}.conv.1.{leaf}"] = (cout,)


def _vr_base(s, p, nin, n, nin_lstm, nout_lstm):
    _vr_cba(s, p + ".enc1", nin, n, 3)
    for i, (cin, cout) in enumerate(((n, 2 * n), (2 * n, 4 * n), (4 * n, 6 * n), (6 * n, 8 * n)), start=2):
        _vr_cba(s, f"{p}.enc{i}.conv1", cin, cout, 3)
        _vr_cba(s, f"{p}.enc{i}.conv2", cout, cout, 3)
    _vr_cba(s, p + ".aspp.conv1.1", 8 * n, 8 * n, 1)
    _vr_cba(s, p + ".aspp.conv2", 8 * n, 8 * n, 1)
    for i in (3, 4, 5):
        _vr_cba(s, f"{p}.aspp.conv{i}", 8 * n, 8 * n, 3)
    _vr_cba(s, p + ".aspp.bottleneck", 40 * n, 8 * n, 1)
    _vr_cba(s, p + ".dec4.conv1", 14 * n, 6 * n, 3)
    _vr_cba(s, p + ".dec3.conv1", 10 * n, 4 * n, 3)
    _vr_cba(s, p + ".dec2.conv1", 6 * n, 2 * n, 3)
    _vr_cba(s, p + ".lstm_dec2.conv", 2 * n, 1, 1)
    hid = nout_lstm // 2
    for suffix in ("", "_reverse"):
        s[f"{p}.lstm_dec2.lstm.weight_ih_l0{suffix}"] = (4 * hid, nin_lstm)
        s[f"{p}.lstm_dec2.lstm.weight_hh_l0{suffix}"] = (4 * hid, hid)
        s[f"{p}.lstm_dec2.lstm.bias_ih_l0{suffix}"] = (4 * hid,)
        s[f"{p}.lstm_dec2.lstm.bias_hh_l0{suffix}"] = (4 * hid,)
    s[p + ".lstm_dec2.dense.0.weight"] = (nin_lstm, nout_lstm)
    s[p + ".lstm_dec2.dense.0.bias"] = (nin_lstm,)
    for leaf in ("weight", "bias", "running_mean", "running_var"):
        s[f"{p}.lstm_dec2.dense.1.{leaf}"] = (nin_lstm,)
    _vr_cba(s, p + ".dec1.conv1", 3 * n + 1, n, 3)


def vr_param_shapes(n_fft=2048, nout=32, nout_lstm=128, is_mono=False):
    """Ordered ``{key: shape}`` of the parameters pd_vr_create takes (include/prodiff_hip.h)."""
    s = OrderedDict()
    nin = 2 if is_mono else 4
    nin_lstm = n_fft // 2 // 2
    _vr_base(s, "stg1_low_band_net.0", nin, nout // 2, nin_lstm // 2, nout_lstm)
    _vr_cba(s, "stg1_low_band_net.1", nout // 2, nout // 4, 1)
    _vr_base(s, "stg1_high_band_net", nin, nout // 4, nin_lstm // 2, nout_lstm // 2)
    _vr_base(s, "stg2_low_band_net.0", nout // 4 + nin, nout, nin_lstm // 2, nout_lstm)
    _vr_cba(s, "stg2_low_band_net.1", nout, nout // 2, 1)
    _vr_base(s, "stg2_high_band_net", nout // 4 + nin, nout // 2, nin_lstm // 2, nout_lstm // 2)
    _vr_base(s, "stg3_full_band_net", 3 * nout // 4 + nin, nout, nin_lstm, nout_lstm)
    s["out.weight"] = (nin, nout, 1, 1)
    s["aux_out.weight"] = (nin, 3 * nout // 4, 1, 1)
    return s


def vr_is_bn(name):
    """The BatchNorm2d after every conv (child 1 of a Conv2DBNActiv's stack) and the LSTM module's BatchNorm1d."""
    return name.rsplit(".", 1)[0].endswith((".conv.1", ".dense.1"))


def synth_vr_tensor(name, shape, seed):
    """The separation model's draw rules: every weight with two or more dimensions (conv, Linear, LSTM) N(0, 1/fan_in),
    BatchNorm gamma and running_var uniform in [0.75, 1.25], BatchNorm beta and running_mean 0.1 N(0, 1), the other
    biases 0.02 N(0, 1)."""
    rng = _rng(seed, name)
    leaf = name.rsplit(".", 1)[-1]
    if vr_is_bn(name) and leaf in ("weight", "running_var"):
        return (0.75 + 0.5 * rng.random(size=shape, dtype=np.float32)).astype(np.float32)
    z = rng.standard_normal(size=shape, dtype=np.float32)
    if vr_is_bn(name):
        return (0.1 * z).astype(np.float32)
    if len(shape) == 1:
        return (0.02 * z).astype(np.float32)
    return (z / np.sqrt(int(np.prod(shape[1:])))).astype(np.float32)


def synth_vr_params(shapes, seed):
    return OrderedDict((k, synth_vr_tensor(k, v, seed)) for k, v in shapes.items())
