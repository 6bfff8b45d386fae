"""The variance-curve and k-th harmonic cases shared by tests/golden/gen_golden_curves.py, the tests and
tools/bench_curves.py: the smallest shapes at which each mechanism can go wrong.

  kth_small     two different rows, k = 0 and 1; unvoiced runs inside and at both ends of f0; f0 two frames short
                (right pad) in row 0 and three frames long (the extra frames feed the interpolation) in row 1
  kth_nyquist   k = 14 and 16: the ``end`` clip at the last bin, frames whose centre lies beyond it (empty mask),
                and a low-f0 row whose centre stays below 1 (empty mask)
  kth_full      the production 44.1 kHz / 2048 / 512 window: 7-8 bins kept among 1025
  kth_hop2      win / hop = 2, the thinnest overlap-add envelope
  curves_voiced_small / curves_voiced_full
                a harmonic stack (amplitudes 1, 0.5, 0.3 on a gliding f0 with vibrato, slow tremolo, -50 dB noise)
                on which the tension ratio is well conditioned (0.3 .. 0.8 on every frame)
  curves_gate   a loud section (rms above -12 dB), a section of exact zeros and a -90 dB section: the top_db floor,
                the amin floor and both ends of the [db_min, db_max] clamp.  Voicing and breath only.

The fixtures store the inputs beside the outputs (the tests read them from there, so a libm's last bit cannot move
them); the ``*_inputs`` functions regenerate them from the seeds for the generator and the CPU tests.
"""
import numpy as np

EDGE_MIN = 1e-3        # bins: distance of center +- half_width (and of center from 1) from the nearest integer
HALF_WIDTH = 3.5

# name -> (samplerate, win, hop, L, ks, per-row f0 lengths relative to the frame count, seed)
KTH = {
    "kth_small": (8000, 256, 64, 64 * 37 + 13, (0, 1), (-2, +3), 301),
    "kth_nyquist": (8000, 256, 64, 64 * 20 + 1, (14, 16), (0, 0), 302),
    "kth_full": (44100, 2048, 512, 512 * 40 + 13, (0,), (0,), 303),
    "kth_hop2": (8000, 256, 128, 128 * 9 + 5, (0,), (0,), 304),
}
# name -> (samplerate, win, hop, f0 frames T (L = hop T + 13), seed)
VOICED = {"curves_voiced_small": (8000, 256, 64, 37, 311), "curves_voiced_full": (44100, 2048, 512, 40, 312)}
GATE = {"curves_gate": (8000, 256, 64, 64 * 37, 321)}
SMOOTH_K = (10, 5)                     # the production kernel (even: 4 left, 5 right) and an odd one
TENSION_DOMAINS = ("ratio", "db", "logit")
TAP_SIZES = (3, 4, 5, 10, 11)


def frames_of(L, hop):
    return L // hop + 1


def mel_lens(L, hop):
    T = frames_of(L, hop)
    return (T, T - 1, T + 2)


def interp_f0(f0):
    """utils/pitch_utils.py:45-51 in f0's own dtype: log2 of the voiced frames (-inf where unvoiced), np.interp
    across the unvoiced ones, 2 ** (.) of every frame."""
    f0 = np.asarray(f0)
    uv = f0 == 0
    with np.errstate(divide="ignore"):
        f = np.log2(f0 + uv)
    f[uv] = -np.inf
    if uv.any() and not uv.all():
        f[uv] = np.interp(np.where(uv)[0], np.where(~uv)[0], f[~uv])
    return 2 ** f


def padded_f0(f0, k, n_samples, hop):
    """binarizer_utils.py:150-153: f0 (k + 1), padded on the right with its last value to the frame count."""
    f = np.asarray(f0) * (k + 1)
    pad = n_samples // hop - len(f) + 1
    if pad > 0:
        f = np.pad(f, (0, pad), mode="constant", constant_values=(f[0], f[-1]))
    return f


def centers(f0, k, n_samples, hop, win, sr):
    """center = f0 * win / sr of every frame, in f0's dtype, as binarizer_utils.py:155-177 computes it."""
    f = interp_f0(padded_f0(f0, k, n_samples, hop))
    return (f * f.dtype.type(win) / f.dtype.type(sr)).astype(f.dtype)


def edge_distance(center, half_width=HALF_WIDTH):
    """The smallest distance of center - hw, center + hw and (center against the threshold 1) from an integer."""
    c = np.asarray(center, np.float64)
    c = c[np.isfinite(c)]
    d = [np.abs(c - half_width - np.round(c - half_width)), np.abs(c + half_width - np.round(c + half_width)),
         np.abs(c - 1.0)]
    return float(np.min(d)) if c.size else np.inf


def _contour(T, base, rng, sr, hop):
    """A gliding f0 with vibrato, float32 [T]."""
    t = np.arange(T) * hop / sr
    cents = 50.0 * np.sin(2 * np.pi * 1.3 * t + rng.uniform(0, 6)) + 480.0 * np.linspace(0, 1, T) * rng.uniform(0.5, 1.0)
    return (base * 2 ** (cents / 1200.0)).astype(np.float32)


def _stack(f0_voiced, L, sr, hop, rng, noise=0.003):
    """Harmonics 1, 0.5, 0.3 on the (interpolated, everywhere positive) contour with a slow tremolo and noise."""
    n = np.arange(L)
    f = np.interp(n / hop, np.arange(len(f0_voiced)), f0_voiced.astype(np.float64))
    ph = 2 * np.pi * np.cumsum(f) / sr
    amp = 0.3 * (0.6 + 0.4 * np.sin(2 * np.pi * 0.9 * n / sr))
    x = amp * (np.sin(ph) + 0.5 * np.sin(2 * ph + 1) + 0.3 * np.sin(3 * ph + 2)) + noise * rng.standard_normal(L)
    return x.astype(np.float32)


def _search(build, check):
    """The first of up to 200 deterministic attempts whose f0 meets the mask-edge condition."""
    for attempt in range(200):
        out = build(attempt)
        if check(out):
            return out
    raise AssertionError("no attempt met the mask-edge condition")


def kth_inputs(name):
    """-> (wavs, f0s): one float32 waveform [L] and one float32 f0 per row."""
    sr, win, hop, L, ks, dlen, seed = KTH[name]
    T = frames_of(L, hop)

    def build(attempt):
        rng = np.random.default_rng(seed * 1000 + attempt)
        wavs, f0s = [], []
        for r, dl in enumerate(dlen):
            n = T + dl
            base = 220.0 if sr == 44100 else 230.0 + 40.0 * r
            if name == "kth_nyquist" and r == 1:
                base = 1.5          # k = 14, 16: center = 1.5 * 15 or 17 * 256 / 8000 < 1 on every frame
            f0 = _contour(n, base, rng, sr, hop)
            if name != "kth_nyquist":
                f0[:2] = 0          # an unvoiced run at the start, inside, and at the end
                f0[7:11] = 0
                f0[n // 2] = 0
                f0[-3:] = 0
            wavs.append(_stack(interp_f0(f0.copy()), L, sr, hop, rng, noise=0.02))
            f0s.append(f0)
        return wavs, f0s

    def check(out):
        return all(edge_distance(centers(f0, k, L, hop, win, sr)) >= 2 * EDGE_MIN for f0 in out[1] for k in ks)

    return _search(build, check)


def voiced_inputs(name):
    """-> (sp, ap, f0): the harmonic stack, a noise with its own envelope, and the f0 (frames 5..8 and 20 unvoiced)."""
    sr, win, hop, T, seed = VOICED[name]
    L = hop * T + 13

    def build(attempt):
        rng = np.random.default_rng(seed * 1000 + attempt)
        t = np.arange(T) * hop / sr
        f0 = (220.0 * 2 ** (0.5 * np.sin(2 * np.pi * 1.3 * t + 0.37 * attempt) / 12 + np.linspace(0, 0.4, T))).astype(np.float32)
        f0[5:9] = 0
        f0[20] = 0
        sp = _stack(interp_f0(f0.copy()), L, sr, hop, rng)
        n = np.arange(L)
        ap = (0.05 * (0.55 + 0.45 * np.sin(2 * np.pi * 1.7 * n / sr)) * rng.standard_normal(L)).astype(np.float32)
        return sp, ap, f0

    def check(out):
        return edge_distance(centers(out[2], 0, L, hop, win, sr)) >= 2 * EDGE_MIN

    return _search(build, check)


def gate_inputs(name):
    """-> (sp, ap): loud / exact zeros / -90 dB sections in two different orders."""
    sr, win, hop, L, seed = GATE[name]
    rng = np.random.default_rng(seed)
    n = np.arange(L)
    loud = 0.6 * np.sin(2 * np.pi * 310.0 * n / sr) + 0.01 * rng.standard_normal(L)
    quiet = 10 ** (-90 / 20) * np.sqrt(2.0) * np.sin(2 * np.pi * 200.0 * n / sr)
    third = L // 3
    sp = np.concatenate([loud[:third], np.zeros(third), quiet[:L - 2 * third]]).astype(np.float32)
    ap = np.concatenate([quiet[:third], 0.05 * loud[:third], np.zeros(L - 2 * third)]).astype(np.float32)
    return sp, ap


def curve_key(kind, smooth_k, mel_len, extra=""):
    """The fixtures' key of one curve: kind voicing / breath / tension_<domain>, smooth_k 0 = unsmoothed."""
    return f"{kind}_s{smooth_k}_m{mel_len}{extra}"
