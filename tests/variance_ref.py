"""TEST INFRASTRUCTURE ONLY: float64 numpy restatement of the variance predictors' forwards, built on
oracle.oracle_encoder (encoder, layer_norm, sinusoid_table, make_positions).  Pinned to the reference's
own outputs (tests/golden/pitchcond_*.npz, dur_*.npz) by tests/test_variance_cpu.py, so the fixtures and
the math are checkable without a GPU.  Nothing in ``prodiff_amd`` imports it.

Follows:
  * PitchPredictor.forward   -- modules/variance_predictor/pitch_predictor.py:57-114
  * NoteEncoder              -- modules/fastspeech/tts_modules.py:332-365
  * DurPredictor.forward     -- modules/variance_predictor/dur_predictor.py:31-36
  * DurationPredictor        -- tts_modules.py:59-132 (LayerNorm eps 1e-12, :45)
"""
import math

import numpy as np

from oracle import oracle_encoder as OE


def _f64(P):
    return {k: np.asarray(v, np.float64) for k, v in P.items()}


def _gather(seq, idx):
    """torch.gather(F.pad(seq, [0, 0, 1, 0]), 1, idx): index 0 is a zero row."""
    B, T, H = seq.shape
    padded = np.concatenate([np.zeros((B, 1, H)), seq], axis=1)
    return np.take_along_axis(padded, idx[..., None].repeat(H, -1), axis=1)


def note_encoder(P, hp, note_midi, note_rest, note_dur):
    """NoteEncoder.forward: x = sqrt(Hn) midi_embed(midi) [!rest] + dur_embed(dur) + sinusoid(positions of
    midi >= 0), then FFTBlocks with the padding mask midi < 0.  Stated through oracle_encoder.encoder: a token
    sequence [midi >= 0] over an all-zero embedding table carries exactly that mask and those positions, and
    the note embedding goes in as extra_embed."""
    Hn = hp["note_hidden_size"]
    x = math.sqrt(Hn) * OE.lin1(P, "note_encoder.note_midi_embed", note_midi) * (~note_rest)[..., None]
    x = x + OE.lin1(P, "note_encoder.note_dur_embed", note_dur)
    Q = {"encoder." + k[len("note_encoder."):]: v for k, v in P.items() if k.startswith("note_encoder.")}
    Q["encoder.embed_tokens.weight"] = np.zeros((2, Hn))
    nhp = dict(hidden_size=Hn, enc_layers=hp["note_layers"], num_heads=hp["note_heads"])
    return OE.encoder(Q, nhp, (note_midi >= 0).astype(np.int64), x)


def pitch_condition(P, hp, txt_tokens, mel2ph, note_midi, note_rest, mel2note, base_pitch, pitch=None,
                    pitch_retake=None, pitch_expr=None, spk_id=None, return_parts=False):
    """PitchPredictor.forward up to the diffusion call -> cond [B, T_mel, H] (float64)."""
    P = _f64(P)
    txt_tokens, mel2ph, mel2note = (np.asarray(v, np.int64) for v in (txt_tokens, mel2ph, mel2note))
    note_midi = np.asarray(note_midi, np.float64)
    note_rest = np.asarray(note_rest, bool)
    dur = OE.mel2ph_to_dur(mel2ph, txt_tokens.shape[1]).astype(np.float64)
    enc = OE.encoder(P, hp, txt_tokens, OE.lin1(P, "dur_embed", dur))
    cond = _gather(enc, mel2ph)
    note_dur = OE.mel2ph_to_dur(mel2note, note_midi.shape[1]).astype(np.float64)
    nenc = note_encoder(P, hp, note_midi, note_rest, note_dur)
    nlin = nenc @ P["note_encode_out_linear.weight"].T + P["note_encode_out_linear.bias"]
    cond = cond + _gather(nlin, mel2note)
    if hp.get("use_spk_id", True):
        cond = cond + P["spk_embed.weight"][np.asarray(spk_id, np.int64).reshape(-1)][:, None, :]
    E = P["pitch_retake_embed.weight"]
    is_retake = pitch_retake is not None
    r = np.asarray(pitch_retake, bool) if is_retake else np.ones(mel2note.shape, bool)
    if pitch_expr is None:
        cond = cond + E[r.astype(np.int64)]
    else:
        e = (np.asarray(pitch_expr, np.float64).reshape(-1, 1) * r)[..., None]
        cond = cond + (E[1] * e + E[0] * (1 - e))
    if is_retake:
        delta = (np.asarray(pitch, np.float64) - np.asarray(base_pitch, np.float64)) * ~r
    else:
        delta = np.zeros(mel2note.shape)
    cond = cond + OE.lin1(P, "delta_pitch_embed", delta)
    return (cond, enc, nlin) if return_parts else cond


def conv1d_same(x, w, b):
    """Conv1d(padding = k // 2) over time-major x [B, T, Cin]; w [Cout, Cin, k]."""
    B, T, _ = x.shape
    k = w.shape[2]
    xp = np.pad(x, ((0, 0), (k // 2, k // 2), (0, 0)))
    y = np.zeros((B, T, w.shape[0]))
    for j in range(k):
        y += xp[:, j:j + T, :] @ np.ascontiguousarray(w[:, :, j].T)   # a strided tap leaves BLAS
    return y + b


def dur_forward(P, hp, txt_tokens, onset, word_dur):
    """DurPredictor.forward(infer=True) -> (durations [B, T], log-domain output [B, T]) (float64)."""
    P = _f64(P)
    txt_tokens = np.asarray(txt_tokens, np.int64)
    extra = P["onset_embed.weight"][np.asarray(onset, np.int64)] + OE.lin1(P, "word_dur_embed",
                                                                            np.asarray(word_dur, np.float64))
    x = OE.encoder(P, hp, txt_tokens, extra)
    mask = (txt_tokens != 0)[..., None].astype(np.float64)
    for i in range(hp["n_layers"]):
        p = f"dur_pred.conv.{i}."
        x = np.maximum(conv1d_same(x, P[p + "1.weight"], P[p + "1.bias"]), 0.0)
        x = OE.layer_norm(x, P[p + "3.weight"], P[p + "3.bias"], eps=1e-12) * mask
    log = ((x @ P["dur_pred.linear.weight"].T + P["dur_pred.linear.bias"]) * mask)[..., 0]
    return np.maximum(np.exp(log) - hp["log_offset"], 0.0), log
