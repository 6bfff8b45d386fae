"""The variance-predictor fixtures (tests/golden/pitchcond_*.npz, dur_*.npz): their definitions, shared by
tests/golden/gen_golden_variance.py (which runs the reference modules) and the tests, and their loaders.
Weights are drawn by prodiff_amd.synth from the stored seed; the files hold inputs, the reference's
outputs and the reference's ordered state-dict key list."""
import numpy as np

from prodiff_amd import synth
from tests import golden_io as G

VOCAB = 40
_SMALL = dict(lengths=[17, 9, 23], note_lengths=[7, 4, 10], pad_tokens=2, pad_notes=1)

# name: hp (over synth.PITCH_DEFAULTS), shapes (synth.synth_pitch_inputs), seeds
PITCH_CASES = {
    # T not a multiple of 8, both paddings, two widths in one handle; a different pitch_expr per row
    "pitchcond_small": dict(hp=dict(enc_layers=2, note_layers=2, num_spk=3), param_seed=301, input_seed=311, **_SMALL),
    # pitch / pitch_retake given: the retake embedding lookup and the delta-pitch term
    "pitchcond_retake": dict(hp=dict(enc_layers=2, note_layers=2, num_spk=3), param_seed=302, input_seed=312,
                             retake=True, **_SMALL),
    # the shipped configuration at a real segment's shape (tests/golden/ds_lengths.json, segment 21)
    "pitchcond_config": dict(hp=dict(num_spk=1), param_seed=303, input_seed=313, lengths=[6], note_lengths=[5],
                             frames=286),
    "pitchcond_nospk": dict(hp=dict(enc_layers=2, note_layers=2, use_spk_id=False), param_seed=304, input_seed=314,
                            **_SMALL),
}

# name: hp (over synth.DUR_DEFAULTS), shapes (synth.synth_dur_inputs), seeds
DUR_CASES = {
    "dur_small": dict(hp=dict(enc_layers=2, n_layers=2, n_chans=128), param_seed=321, input_seed=331,
                      lengths=[17, 9, 23], pad_tokens=2),
    "dur_config": dict(hp=dict(), param_seed=322, input_seed=332, lengths=[24], pad_tokens=0),
}
# dur_pred.linear.bias of the duration fixtures: the head's output is ~N(0, 1) with synthetic weights, so
# exp(v) - 1 would be clamped to 0 on half the tokens at bias ~0; the generator asserts that the reference's
# own output is > 0 on at least half of the non-padding tokens with this value
DUR_BIAS = 1.0

PITCH_INPUTS = ("txt_tokens", "mel2ph", "note_midi", "note_rest", "mel2note", "base_pitch", "pitch", "pitch_retake",
                "pitch_expr", "spk_id")
DUR_INPUTS = ("txt_tokens", "onset", "word_dur")


def pitch_hp(name):
    return dict(synth.PITCH_DEFAULTS, **PITCH_CASES[name]["hp"])


def dur_hp(name):
    return dict(synth.DUR_DEFAULTS, **DUR_CASES[name]["hp"])


def pitch_params(name):
    c = PITCH_CASES[name]
    return synth.synth_variance_params(synth.pitch_param_shapes(VOCAB, **pitch_hp(name)), c["param_seed"])


def dur_params(name):
    c = DUR_CASES[name]
    return synth.synth_variance_params(synth.dur_param_shapes(VOCAB, **dur_hp(name)), c["param_seed"], DUR_BIAS)


def pitch_inputs(name):
    c = PITCH_CASES[name]
    hp = pitch_hp(name)
    x = synth.synth_pitch_inputs(c["input_seed"], c["lengths"], c["note_lengths"], VOCAB, hp["num_spk"],
                                 c.get("pad_tokens", 0), c.get("pad_notes", 0), c.get("frames"),
                                 c.get("retake", False))
    if not hp["use_spk_id"]:
        x.pop("spk_id")
    return x


def dur_inputs(name):
    c = DUR_CASES[name]
    return synth.synth_dur_inputs(c["input_seed"], c["lengths"], VOCAB, c["pad_tokens"])


def reference_pitch_hparams(hp):
    """The reference PitchPredictor's hparams for a case's hp (a one-layer WaveNet: cond is captured before it)."""
    return dict(hidden_size=hp["hidden_size"], enc_layers=hp["enc_layers"],
                enc_ffn_kernel_size=hp["enc_ffn_kernel_size"], num_heads=hp["num_heads"], dropout=0.1,
                use_dur_embed=True, use_spk_id=hp["use_spk_id"], datasets=["d%d" % i for i in range(hp["num_spk"])],
                sampling_algorithm="euler",
                f0_prediction_args=dict(spec_min=-8.0, spec_max=8.0, clamp_min=-12.0, clamp_max=12.0, repeat_bins=8,
                                        encoder_args=dict(hidden_size=hp["note_hidden_size"],
                                                          num_layers=hp["note_layers"],
                                                          ffn_kernel_size=hp["note_ffn_kernel_size"],
                                                          num_heads=hp["note_heads"]),
                                        denoise_args=dict(dilation_cycle_length=1, residual_layers=1,
                                                          residual_channels=64),
                                        timesteps=4, timescale=1000))


def reference_dur_hparams(hp):
    return dict(hidden_size=hp["hidden_size"], enc_layers=hp["enc_layers"],
                enc_ffn_kernel_size=hp["enc_ffn_kernel_size"], num_heads=hp["num_heads"],
                dur_prediction_args=dict(num_layers=hp["n_layers"], hidden_size=hp["n_chans"], dropout=0.1,
                                         kernel_size=hp["kernel_size"], log_offset=hp["log_offset"], loss_type="mse"))


def pitch_case(name):
    """(hp, params, inputs, fixture) of tests/golden/<name>.npz."""
    d = G.load(name)
    return pitch_hp(name), pitch_params(name), {k: d[k] for k in PITCH_INPUTS if k in d}, d


def dur_case(name):
    d = G.load(name)
    return dur_hp(name), dur_params(name), {k: d[k] for k in DUR_INPUTS}, d


def lens_of(name):
    """(txt_lens, note_lens or None) of a case's rows."""
    c = PITCH_CASES.get(name) or DUR_CASES[name]
    return list(c["lengths"]), (list(c["note_lengths"]) if "note_lengths" in c else None)


def row_alone(ins, b, n_tok, n_note=None):
    """Row b of a padded batch as the segment alone: its own tokens / notes / frames only."""
    out = {}
    frames = int((ins["mel2ph"][b] > 0).sum()) if "mel2ph" in ins else None
    for k, v in ins.items():
        r = v[b:b + 1]
        if k in ("txt_tokens", "onset", "word_dur"):
            r = r[:, :n_tok]
        elif k in ("note_midi", "note_rest"):
            r = r[:, :n_note]
        elif k in ("mel2ph", "mel2note", "base_pitch", "pitch", "pitch_retake"):
            r = r[:, :frames]
        out[k] = np.ascontiguousarray(r)
    return out
