"""Generate the mel-analysis fixtures (tests/golden/mel_*.npz) from the REFERENCE's
modules/nsf_hifigan/nvSTFT.py:STFT.get_mel, run on the CPU.

Runs only where the reference checkout exists (REF below):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_mel.py

librosa is not installed there, so ``sys.modules`` gets a stub whose ``filters.mel`` is
``prodiff_amd.mel.mel_filterbank`` (the same kind of shim as the chardet stub in gen_golden.py:32).
The filterbank is therefore NOT pinned to librosa by these fixtures: tests/test_mel_cpu.py pins it
by its properties, and every fixture stores the basis the reference used.

Each fixture holds the wav [B, L], the reference's log-mel [B, n_mels, T] and magnitude spectrum
[B, n_fft//2 + 1, T] (the second operand of nvSTFT.py:95's matmul, recorded), the basis and the settings.
The signals come from tests/mel_ref.py (seeded).
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

from prodiff_amd.mel import mel_filterbank  # noqa: E402
from tests import mel_ref as R              # noqa: E402

librosa = types.ModuleType("librosa")
librosa.filters = types.ModuleType("librosa.filters")
librosa.filters.mel = lambda sr, n_fft, n_mels, fmin, fmax: mel_filterbank(sr, n_fft, n_mels, fmin, fmax)
sys.modules.setdefault("librosa", librosa)
sys.modules.setdefault("librosa.filters", librosa.filters)
torch.set_num_threads(8)

import modules.nsf_hifigan.nvSTFT as nv  # noqa: E402


def run_case(name):
    cfg, keyshift, speed, L, kinds = R.CASES[name]
    wav = R.case_wav(name)
    stft = nv.STFT(cfg["sr"], cfg["n_mels"], cfg["n_fft"], cfg["win_size"], cfg["hop_length"], cfg["fmin"], cfg["fmax"])
    seen = []
    matmul = torch.matmul

    def recording_matmul(a, b):
        seen.append(b.clone())
        return matmul(a, b)

    torch.matmul = recording_matmul
    try:
        with torch.no_grad():
            mel = stft.get_mel(torch.from_numpy(wav), keyshift=keyshift, speed=speed)
    finally:
        torch.matmul = matmul
    assert len(seen) == 1
    basis = next(iter(stft.mel_basis.values())).numpy()
    out = dict(wav=wav, mel=mel.numpy(), spec=seen[0].numpy(), basis=basis, keyshift=np.float64(keyshift),
               speed=np.float64(speed), cfg_keys=np.array(list(cfg)), cfg_vals=np.array([cfg[k] for k in cfg], np.int64),
               kinds=np.array(kinds))
    assert mel.shape == (len(kinds), cfg["n_mels"], R.num_frames(L, cfg, keyshift, speed)), mel.shape
    path = os.path.join(HERE, f"mel_{name}.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < (1 << 20), (path, os.path.getsize(path))
    print(f"{name}: mel {mel.shape} spec {tuple(seen[0].shape)} {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    for name in (sys.argv[1:] or R.CASES):
        run_case(name)
