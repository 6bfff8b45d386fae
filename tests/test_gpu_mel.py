"""GPU tests of the mel analysis (pd_mel through prodiff_amd.mel.STFT and NsfHifiGAN.wav2spec) against the
reference's own outputs (tests/golden/mel_*.npz, made by tests/golden/gen_golden_mel.py from
modules/nsf_hifigan/nvSTFT.py) and the float64 restatement tests/mel_ref.py.

Two bars per case:
 (i)  magnitude spectrum against the reference's: |d| <= 1e-5 * max_k |ref[t]| per frame (the project's waveform
      bar, per frame);
 (ii) log-mel against float64: with e_ref = max|reference - f64| and e_hip = max|native - f64| of the case,
      e_hip <= 4 e_ref + 2e-6.  A flat bar on the log is wrong: two float32 methods differ by 3e-4 in quiet mel
      bands of the harmonic signals while agreeing to 5e-7 in the linear spectrum.  The factor 4: the fmaf chain
      over K <= 4096 rounds more often than an FFT's log2 N stages; 2e-6 is two ulps of log(clip).
"""
import functools
import struct

import numpy as np
import pytest
import torch

from prodiff_amd import STFT, _lib
from prodiff_amd.mel import num_frames as mel_frames
from prodiff_amd.nsf_hifigan import NsfHifiGAN
from tests import mel_ref as R

pytestmark = pytest.mark.gpu

LOG_CLIP = float(np.log(1e-5))
LN_TO_LOG10 = 0.434294


@functools.lru_cache(maxsize=None)
def stft(cfg_name):
    """One STFT per settings for the whole session: its handles (one per key shift and speed) are reused."""
    cfg = {"SVS": R.SVS, "TTS": R.TTS, "SHORT_WIN": R.SHORT_WIN}[cfg_name]
    return STFT(cfg["sr"], cfg["n_mels"], cfg["n_fft"], cfg["win_size"], cfg["hop_length"], cfg["fmin"], cfg["fmax"])


def stft_of(cfg):
    return stft("SVS" if cfg is R.SVS else "TTS" if cfg is R.TTS else "SHORT_WIN")


def cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


# ---------------------------------------------------------------- a. parity
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_parity_with_the_reference(name):
    cfg, keyshift, speed, L, kinds = R.CASES[name]
    d = R.fixture(name)
    mel64, _, _ = R.restated(name)
    s = stft_of(cfg)
    np.testing.assert_array_equal(s.mel_basis_host.numpy(), d["basis"])
    mel, spec = s.get_mel_time_major(cuda(d["wav"]), keyshift, speed, return_spec=True)
    assert mel.shape == (len(kinds), d["mel"].shape[2], cfg["n_mels"])
    ref_layout = s.get_mel(cuda(d["wav"]), keyshift, speed)
    assert ref_layout.shape == d["mel"].shape and torch.equal(ref_layout, mel.transpose(1, 2))
    mel = mel.cpu().numpy().transpose(0, 2, 1)
    spec = spec.cpu().numpy().transpose(0, 2, 1)
    assert np.isfinite(mel).all() and np.isfinite(spec).all()
    peak = np.abs(d["spec"]).max(axis=1, keepdims=True)
    d_spec = np.abs(spec - d["spec"])
    e_ref = float(np.abs(d["mel"] - mel64).max())
    e_hip = float(np.abs(mel - mel64).max())
    print(f"{name}: spectrum max|d| / frame peak = {float((d_spec / np.where(peak > 0, peak, 1.0)).max()):.2e}, "
          f"e_ref = {e_ref:.2e}, e_hip = {e_hip:.2e}, max|native - reference| = {float(np.abs(mel - d['mel']).max()):.2e}")
    assert (d_spec <= 1e-5 * peak).all()
    assert e_hip <= 4 * e_ref + 2e-6


# ---------------------------------------------------------------- b. ragged batch
def ragged_batch():
    lens = [769, 5 * 512 + 100, 33 * 512]
    L = max(lens)
    wav = np.zeros((3, L), np.float32)
    for i, (n, kind) in enumerate(zip(lens, ("noise", "harmonic", "quiet"))):
        wav[i, :n] = R.make_signal(kind, n, 44100, 900 + i)
        wav[i, n:] = 0.5                                      # what lies past a row's length must not be read
    return wav, lens


def test_ragged_rows_equal_the_rows_alone():
    s = stft("SVS")
    wav, lens = ragged_batch()
    alone = [s.get_mel_time_major(cuda(wav[i:i + 1, :n])) for i, n in enumerate(lens)]
    for order in ([0, 1, 2], [2, 0, 1], [1, 2, 0]):
        out = s.get_mel_time_major(cuda(wav[order]), lens=[lens[i] for i in order])
        for row, i in enumerate(order):
            T = alone[i].shape[1]
            assert T == 1 + (lens[i] - 512) // 512
            assert torch.equal(out[row, :T], alone[i][0]), (order, i)
    # the lengths as a device tensor
    out = s.get_mel_time_major(cuda(wav), lens=torch.tensor(lens, dtype=torch.int32).cuda())
    for i in range(3):
        assert torch.equal(out[i, :alone[i].shape[1]], alone[i][0])


# ---------------------------------------------------------------- c. key shifts
@pytest.mark.parametrize("keyshift,nb", [(-7, 684), (-12, 513), (7, 1025)])
def test_key_shift_bins_and_clipped_bands(keyshift, nb):
    """Bins from nb = min(n_fft/2, nf/2) + 1 on are exactly zero in spec_out; mel bands that see only those
    bins, and every band of an all-zero frame, equal out_scale * log(clip) within 2e-6."""
    s = stft("SVS")
    L = 12 * 512
    wav = np.stack([R.make_signal("zeros", L, 44100, 77), R.make_signal("noise", L, 44100, 78)])
    wav[0, :] = 0.0
    mel, spec = s.get_mel_time_major(cuda(wav), keyshift, 1, out_scale=LN_TO_LOG10, return_spec=True)
    mel, spec = mel.cpu().numpy(), spec.cpu().numpy()
    assert spec.shape[2] == 1025 and (spec[1, :, :nb] > 0).all()
    assert (spec[:, :, nb:] == 0).all() and (spec[0] == 0).all()
    assert np.abs(mel[0] - LN_TO_LOG10 * LOG_CLIP).max() <= 2e-6
    dead = ~(s.mel_basis_host.numpy()[:, :nb] > 0).any(axis=1)          # bands whose filters lie above nb
    assert dead.any() == (keyshift < 0)
    assert np.abs(mel[1][:, dead] - LN_TO_LOG10 * LOG_CLIP).max(initial=0.0) <= 2e-6
    live = s.mel_basis_host.numpy()[:, :nb].sum(axis=1) > 1e-3
    assert (mel[1][:, live] > LN_TO_LOG10 * LOG_CLIP + 1e-3).all()


# ---------------------------------------------------------------- d. malformed arguments
def test_malformed_lens_are_clamped():
    """A lens entry out of range is clamped in the kernel: no error, and the other rows are bit-identical
    to the clean batch.  This only exercises the clamps."""
    s = stft("SVS")
    L = 6 * 512
    wav = cuda(np.stack([R.make_signal(k, L, 44100, 50 + i) for i, k in enumerate(("noise", "harmonic", "noise"))]))
    clean = s.get_mel_time_major(wav)
    for bad in (-5, 0, 768, L + 1, 10 ** 6, -2 ** 31):
        out = s.get_mel_time_major(wav, lens=torch.tensor([L, bad, L], dtype=torch.int64).to(torch.int32).cuda())
        assert torch.equal(out[0], clean[0]) and torch.equal(out[2], clean[2]), bad
    torch.cuda.synchronize()


def test_short_signals_and_null_pointers_are_refused():
    s = stft("SVS")
    lib = _lib.lib()
    wav = torch.zeros(1, 4096, device="cuda")
    h = s.handle(0, 1, wav.device)
    assert lib.pd_mel_min_samples(h) == 769 and lib.pd_mel_frames(h, 769) == 1 and lib.pd_mel_frames(h, 768) == 0
    assert lib.pd_mel_frames(h, 12 * 512 + 37) == 12 and lib.pd_mel_workspace_size(h, 8, 4096) == 0
    out = torch.zeros(1, 8, 128, device="cuda")
    st = _lib.stream_ptr(wav.device)
    assert lib.pd_mel_forward(h, _lib.fptr(wav), None, 1.0, _lib.fptr(out), None, 1, 768, None, 0, st) == 1
    assert b"pd_mel_min_samples" in lib.pd_last_error()
    assert lib.pd_mel_forward(h, None, None, 1.0, _lib.fptr(out), None, 1, 4096, None, 0, st) == 1
    assert lib.pd_mel_forward(h, _lib.fptr(wav), None, 1.0, None, None, 1, 4096, None, 0, st) == 1
    assert lib.pd_mel_forward(None, _lib.fptr(wav), None, 1.0, _lib.fptr(out), None, 1, 4096, None, 0, st) == 1
    assert lib.pd_mel_forward(h, _lib.fptr(wav), None, 1.0, _lib.fptr(out), None, 0, 4096, None, 0, st) == 1
    torch.cuda.synchronize()
    assert (out == 0).all()
    with pytest.raises(ValueError, match="at least 769"):
        s.get_mel(wav[:, :768])
    with pytest.raises(ValueError, match="at least 1793"):
        s.get_mel(wav[:, :1792], keyshift=12)


# ---------------------------------------------------------------- e. lifecycle
def test_handles_are_per_key_shift_and_speed_and_freed():
    lib = _lib.lib()
    torch.cuda.synchronize()
    start = lib.pd_live_device_bytes()
    s = STFT(**R.TTS)
    wav = cuda(R.make_signal("noise", 3000, 22050, 5)[None])
    a = s.get_mel(wav)
    one = lib.pd_live_device_bytes()
    assert one >= start + 2 * 1024 * 513 * 4          # the two DFT tables at least
    b = s.get_mel(wav, keyshift=2, speed=1.5)
    two = lib.pd_live_device_bytes()
    assert two > one and len(s.handles) == 2
    assert len({nh.h.value for nh in s.handles.values()}) == 2
    assert torch.equal(s.get_mel(wav), a) and lib.pd_live_device_bytes() == two      # the first handle is reused
    assert a.shape[2] != b.shape[2]
    s.close()
    assert lib.pd_live_device_bytes() == start and not s.handles


def test_eviction_frees_the_evicted_handle():
    """Nine speeds on an STFT that keeps eight handles: the ninth create closes the oldest handle, so the live
    device bytes stay where they were after the eighth (every pool is the same size: the tables depend on n_fft
    and n_mels only)."""
    lib = _lib.lib()
    torch.cuda.synchronize()
    start = lib.pd_live_device_bytes()
    s = STFT(sr=22050, n_mels=8, n_fft=64, win_size=64, hop_length=16, fmin=0, fmax=11025)
    wav = cuda(R.make_signal("noise", 400, 22050, 7)[None])
    live = []
    for k in range(16, 25):                     # hops 16 .. 24
        assert s.get_mel(wav, speed=k / 16).shape[2] == mel_frames(400, 64, 64, 16, 0, k / 16)
        live.append(lib.pd_live_device_bytes())
    per = live[0] - start
    assert per > 0 and live[:8] == [start + (i + 1) * per for i in range(8)]
    assert live[8] == live[7] and len(s.handles) == 8
    assert (0.0, 1.0, str(wav.device)) not in s.handles and (0.0, 17 / 16, str(wav.device)) in s.handles
    s.close()
    assert lib.pd_live_device_bytes() == start and not s.handles


# ---------------------------------------------------------------- f. hipGraph
def test_captured_get_mel_replays_bit_identically():
    s = stft("SVS")
    wav = cuda(np.stack([R.make_signal("harmonic", 40 * 512 + 3, 44100, 60), R.make_signal("noise", 40 * 512 + 3, 44100, 61)]))
    eager = s.get_mel(wav, keyshift=-7).clone()          # also builds the handle before the capture
    torch.cuda.synchronize()
    static = torch.zeros_like(wav)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = s.get_mel(static, keyshift=-7)
    static.copy_(wav)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    static.copy_(wav.flip(0))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager.flip(0))


# ---------------------------------------------------------------- g. wav2spec
def test_wav2spec_reads_a_stereo_pcm16_file(tmp_path):
    hp = dict(audio_sample_rate=44100, audio_num_mel_bins=128, fft_size=2048, win_size=2048, hop_size=512, fmin=40,
              fmax=16000)
    n = 9 * 512 + 11
    x = np.stack([R.make_signal("harmonic", n, 44100, 70), R.make_signal("noise", n, 44100, 71)], axis=1)
    pcm = np.round(x.astype(np.float64) * 32767).astype("<i2")
    fmt = struct.pack("<HHIIHH", 1, 2, 44100, 44100 * 4, 4, 16)
    raw = pcm.tobytes()
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(raw)) + raw
    path = str(tmp_path / "stereo.wav")
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)
    mono = (pcm.astype(np.float32) / 32768.0).mean(axis=1, dtype=np.float64).astype(np.float32)
    for keyshift, speed in ((0, 1), (-3, 1.25)):
        wav, mel = NsfHifiGAN.wav2spec(path, hp, keyshift=keyshift, speed=speed)
        assert isinstance(wav, np.ndarray) and isinstance(mel, np.ndarray)
        np.testing.assert_array_equal(wav, mono)
        want = stft("SVS").get_mel(cuda(mono[None]), keyshift, speed)[0].T
        assert mel.shape == tuple(want.shape) and mel.shape[1] == 128
        tm = stft("SVS").get_mel_time_major(cuda(mono[None]), keyshift, speed, out_scale=LN_TO_LOG10)[0]
        np.testing.assert_array_equal(mel, tm.cpu().numpy())
        np.testing.assert_allclose(mel, LN_TO_LOG10 * want.cpu().numpy(), rtol=0, atol=2e-6)
    wav2, mel2 = NsfHifiGAN.wav2spec(mono, hp)           # an array instead of a path
    np.testing.assert_array_equal(wav2, mono)
    assert mel2.shape == (1 + (n - 512) // 512, 128)
