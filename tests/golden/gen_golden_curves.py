"""Generate the variance-curve fixtures (tests/golden/kth_*.npz, curves_*.npz) from the REFERENCE's
component/binarizer/binarizer_utils.py (get_energy, get_voicing, get_breath, get_kth_harmonic, get_tension) and
modules/commons/common_layers.py:SinusoidalSmoothingConv1d, run on the CPU in float32 and, with the same inputs cast
to double, in float64.

Runs only where the reference checkout exists; PRODIFF_REFERENCE names its root:

    PRODIFF_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_curves.py

librosa is not installed here.  The two librosa functions the reference calls, ``feature.rms`` and
``amplitude_to_db``, are put into ``sys.modules`` as a stand-in module holding tests/curves_ref.py's restatement of
librosa 0.8.0 (the version the reference pins): that part of the golden is OUR restatement of librosa, not librosa.
Everything else -- the frame padding and cutting, the tension arithmetic, interp_f0, the mask, torch.stft / istft,
the smoothing module and its taps -- is the reference's own code.  The packages whose __init__ import absent
libraries (component, component.binarizer, utils, modules, modules.vr, modules.nsf_hifigan.nvSTFT,
utils.text_encoder) are replaced by bare packages or empty stand-ins, as gen_golden_vr.py does for modules.vr.

Each fixture stores its inputs, the float32 run, the float64 run (suffix 64) and, for the conditions the tests assert
again, the reference's centres (``center*``) and its unsmoothed tension ratio.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ["PRODIFF_REFERENCE"]
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

from tests import curves_cases as CC   # noqa: E402
from tests import curves_ref as CR     # noqa: E402
from tests import golden_io            # noqa: E402


def bare_package(name, *path):
    m = types.ModuleType(name)
    m.__path__ = [os.path.join(REF, *path)]
    sys.modules[name] = m


def stand_in(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m


for _name in ("component", "component.binarizer", "utils", "modules", "modules.nsf_hifigan"):
    bare_package(_name, *_name.split("."))
stand_in("modules.vr", load_sep_model=None)
stand_in("modules.nsf_hifigan.nvSTFT", STFT=None)
stand_in("utils.text_encoder", TokenTextEncoder=None)
stand_in("librosa", amplitude_to_db=CR.amplitude_to_db,
         feature=types.SimpleNamespace(rms=lambda y, frame_length, hop_length: CR.rms(y, frame_length, hop_length)[None]))
torch.set_num_threads(8)

BU = importlib.import_module("component.binarizer.binarizer_utils")
from modules.commons.common_layers import SinusoidalSmoothingConv1d   # noqa: E402
from utils.pitch_utils import interp_f0                               # noqa: E402

torch.cuda.is_available = lambda: False     # get_kth_harmonic picks its device by itself: force the CPU


def smoother(k, dtype):
    if not k:
        return lambda x: x
    conv = SinusoidalSmoothingConv1d(k)
    return conv.double() if dtype == np.float64 else conv


def ref_center(k, f0, n, hop, win, sr):
    """The reference's own centre of every frame (binarizer_utils.py:150-177), in f0's dtype."""
    f = f0 * (k + 1)
    pad = n // hop - len(f) + 1
    if pad > 0:
        f = np.pad(f, (0, pad), mode="constant", constant_values=(f[0], f[-1]))
    f, _ = interp_f0(f, uv=f == 0)
    return (torch.from_numpy(f) * win / sr).numpy()


def gen_kth(name):
    sr, win, hop, L, ks, _, seed = CC.KTH[name]
    wavs, f0s = CC.kth_inputs(name)
    arrays = dict(seed=np.int64(seed))
    worst, edge = 0.0, np.inf
    for r, (wav, f0) in enumerate(zip(wavs, f0s)):
        arrays[f"wav{r}"], arrays[f"f0{r}"] = wav, f0
        for k in ks:
            y = BU.get_kth_harmonic(k, wav, f0.copy(), hop, win, sr)
            y64 = BU.get_kth_harmonic(k, wav.astype(np.float64), f0.astype(np.float64), hop, win, sr)
            c = ref_center(k, f0.copy(), L, hop, win, sr)
            assert y.dtype == np.float32 and y64.dtype == np.float64 and c.dtype == np.float32
            np.testing.assert_array_equal(c, CC.centers(f0, k, L, hop, win, sr))
            edge = min(edge, CC.edge_distance(c))
            peak = np.abs(y64).max()
            if peak > 0:
                worst = max(worst, float(np.abs(y - y64).max() / peak))
            arrays[f"y{r}_k{k}"], arrays[f"y64_{r}_k{k}"], arrays[f"center{r}_k{k}"] = y, y64, c
    assert edge >= CC.EDGE_MIN, (name, edge)
    paths = golden_io.save(name, arrays)
    print(f"{name}: mask edge distance {edge:.2e}  e_ref / peak {worst:.2e}  files {[os.path.getsize(p) for p in paths]}")


def curves_of(sp, ap, f0, sr, win, hop, dtype, arrays, suffix, with_tension, pad_modes=("reflect",), norms=(True,)):
    L = len(sp)
    sp, ap = sp.astype(dtype), ap.astype(dtype)
    f0 = None if f0 is None else f0.astype(dtype)
    for pad_mode in pad_modes:
        # the stand-in's pad mode is the only thing a newer librosa changes
        sys.modules["librosa"].feature.rms = \
            lambda y, frame_length, hop_length, pm=pad_mode: CR.rms(y, frame_length, hop_length, pm)[None]
        for mel_len in CC.mel_lens(L, hop):
            for k in (0,) + CC.SMOOTH_K:
                sm = smoother(k, dtype)
                for norm in norms:
                    extra = ("" if pad_mode == "reflect" else "_constant") + ("" if norm else "_raw") + suffix
                    arrays[CC.curve_key("voicing", k, mel_len, extra)] = \
                        BU.get_voicing(sp, mel_len, hop, win, sm, norm=norm, device="cpu")
                    arrays[CC.curve_key("breath", k, mel_len, extra)] = \
                        BU.get_breath(ap, mel_len, hop, win, sm, norm=norm, device="cpu")
                if with_tension:
                    for domain in CC.TENSION_DOMAINS:
                        arrays[CC.curve_key("tension_" + domain, k, mel_len, suffix)] = \
                            BU.get_tension(sp, mel_len, f0.copy(), hop, win, sr, sm, domain=domain, device="cpu")
    sys.modules["librosa"].feature.rms = lambda y, frame_length, hop_length: CR.rms(y, frame_length, hop_length)[None]


def report(name, arrays):
    e = {}
    for key in [k for k in arrays if k.endswith("64") and k[:-2] in arrays]:
        kind = key.split("_s")[0]
        e[kind] = max(e.get(kind, 0.0), float(np.abs(arrays[key[:-2]] - arrays[key]).max()))
    paths = golden_io.save(name, arrays)
    print(f"{name}: e_ref " + "  ".join(f"{k} {v:.2e}" for k, v in e.items()) +
          f"  files {[os.path.getsize(p) for p in paths]}")


def gen_voiced(name):
    sr, win, hop, T, seed = CC.VOICED[name]
    sp, ap, f0 = CC.voiced_inputs(name)
    L = len(sp)
    arrays = dict(seed=np.int64(seed), sp=sp, ap=ap, f0=f0)
    c = ref_center(0, f0.copy(), L, hop, win, sr)
    edge = CC.edge_distance(c)
    assert edge >= CC.EDGE_MIN, (name, edge)
    arrays["center"] = c
    base = BU.get_kth_harmonic(0, sp, f0.copy(), hop, win, sr)
    base64 = BU.get_kth_harmonic(0, sp.astype(np.float64), f0.astype(np.float64), hop, win, sr)
    arrays["base"], arrays["base64"] = base, base64
    curves_of(sp, ap, f0, sr, win, hop, np.float32, arrays, "", True)
    curves_of(sp, ap, f0, sr, win, hop, np.float64, arrays, "64", True)
    ratio = arrays[CC.curve_key("tension_ratio", 0, CC.frames_of(L, hop))]
    assert ratio.min() >= 0.3 and ratio.max() <= 0.8, (name, ratio.min(), ratio.max())
    print(f"{name}: mask edge distance {edge:.2e}  tension ratio in [{ratio.min():.3f}, {ratio.max():.3f}]  "
          f"base e_ref / peak {np.abs(base - base64).max() / np.abs(base64).max():.2e}")
    report(name, arrays)


def gen_gate(name):
    sr, win, hop, L, seed = CC.GATE[name]
    sp, ap = CC.gate_inputs(name)
    arrays = dict(seed=np.int64(seed), sp=sp, ap=ap)
    for dtype, suffix in ((np.float32, ""), (np.float64, "64")):
        curves_of(sp, ap, None, sr, win, hop, dtype, arrays, suffix, False, ("reflect", "constant"), (True, False))
    raw = arrays[CC.curve_key("voicing", 0, CC.frames_of(L, hop), "_raw")]
    e = CR.get_energy(sp, CC.frames_of(L, hop), hop, win, "amplitude")
    assert 20 * np.log10(e.max()) > -12.0 and (e == 0).any(), (e.max(), e.min())
    assert raw.max() > -12.0 and raw.min() == raw.max() - 80.0, (raw.min(), raw.max())       # the top_db floor
    braw = arrays[CC.curve_key("breath", 0, CC.frames_of(L, hop), "_raw")]
    assert braw.max() < -20.0 and abs(braw.min() + 100.0) < 1e-3, (braw.min(), braw.max())          # the amin floor
    print(f"{name}: voicing dB in [{raw.min():.1f}, {raw.max():.1f}]  breath dB in [{braw.min():.1f}, {braw.max():.1f}]")
    report(name, arrays)


def main():
    taps = {f"taps{k}": SinusoidalSmoothingConv1d(k).weight.detach().numpy().reshape(-1) for k in CC.TAP_SIZES}
    golden_io.save("curves_taps", taps)
    for name in CC.KTH:
        gen_kth(name)
    for name in CC.VOICED:
        gen_voiced(name)
    for name in CC.GATE:
        gen_gate(name)


if __name__ == "__main__":
    main()
