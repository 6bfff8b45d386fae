"""A numpy / torch CPU restatement of the variance curves and the k-th harmonic isolation
(component/binarizer/binarizer_utils.py:115-213 with librosa 0.8.0's feature.rms and amplitude_to_db), in the dtype
of its inputs: float32 performs the reference's float32 operations, float64 is the yardstick.  No reference import.
``kth_harmonic_sparse`` is the form the kernels compute: only the kept bins, the inverse as a sum of windowed
sinusoids over the covering frames.
"""
import numpy as np
import torch
import torch.nn.functional as F

from tests.curves_cases import interp_f0, padded_f0


# ---------------------------------------------------------------- librosa 0.8.0, restated
def rms(y, frame_length, hop_length, pad_mode="reflect"):
    """librosa.feature.rms(y=, frame_length=, hop_length=, center=True)[0]: util.frame's strided view (the frame
    axis contiguous), mean of squares over it, square root; in y's dtype."""
    y = np.pad(np.asarray(y), int(frame_length // 2), mode=pad_mode)
    n = 1 + (len(y) - frame_length) // hop_length
    x = np.lib.stride_tricks.as_strided(y, shape=(frame_length, n), strides=(y.itemsize, hop_length * y.itemsize))
    return np.sqrt(np.mean(np.abs(x) ** 2, axis=0))


def amplitude_to_db(S, ref=1.0, amin=1e-5, top_db=80.0):
    """librosa.amplitude_to_db -> power_to_db(S ** 2, ref ** 2, amin ** 2, top_db)."""
    power = np.square(np.abs(np.asarray(S)))
    log_spec = 10.0 * np.log10(np.maximum(amin ** 2, power))
    log_spec -= 10.0 * np.log10(np.maximum(amin ** 2, np.abs(ref) ** 2))
    return np.maximum(log_spec, log_spec.max() - top_db)


# ---------------------------------------------------------------- binarizer_utils.py
def get_energy(waveform, mel_len, hop_size, win_size, domain="db", pad_mode="reflect"):
    energy = rms(waveform, win_size, hop_size, pad_mode)
    if len(energy) < mel_len:
        energy = np.pad(energy, (0, mel_len - len(energy)))
    energy = energy[:mel_len]
    if domain == "db":
        return amplitude_to_db(energy)
    if domain == "amplitude":
        return energy
    raise ValueError(f"Unknown domain: {domain}")


def smoothing_taps(kernel_size):
    k = torch.sin(torch.from_numpy(np.linspace(0, 1, kernel_size).astype(np.float32) * np.pi))
    k /= k.sum()
    return k.numpy()


def smooth(x, kernel_size):
    """SinusoidalSmoothingConv1d(kernel_size) on a curve [T], in x's dtype (the float32 taps cast to it)."""
    if not kernel_size:
        return np.asarray(x)
    t = torch.from_numpy(np.ascontiguousarray(x))
    w = torch.from_numpy(smoothing_taps(kernel_size)).to(t.dtype)
    total = kernel_size - 1
    xp = F.pad(t[None, None], (total // 2, total - total // 2), mode="replicate")
    return F.conv1d(xp, w[None, None])[0, 0].numpy()


def db_curve(wav, mel_len, hop_size, win_size, kernel_size, norm=True, db_min=-96.0, db_max=-12.0, pad_mode="reflect"):
    """get_voicing / get_breath."""
    v = torch.from_numpy(smooth(get_energy(wav, mel_len, hop_size, win_size, pad_mode=pad_mode), kernel_size))
    if norm:
        v = (torch.clamp(v, db_min, db_max) - db_min) / (db_max - db_min)
    return v.numpy()


def nuttall(win_size, dtype):
    phase = torch.arange(win_size, dtype=dtype) / win_size * 2 * np.pi
    return 0.355768 - 0.487396 * torch.cos(phase) + 0.144232 * torch.cos(2 * phase) - 0.012604 * torch.cos(3 * phase)


def kth_mask(k, f0, n_samples, hop_size, win_size, samplerate, half_width=3.5):
    """-> (center [T_f0'], mask [T_f0', n_bins]) as binarizer_utils.py:150-180, in f0's dtype."""
    f = torch.from_numpy(interp_f0(padded_f0(f0, k, n_samples, hop_size)))[:, None]
    n_bins = win_size // 2 + 1
    idx = torch.arange(n_bins)[None].to(f)
    center = f * win_size / samplerate
    start = torch.clip(center - half_width, min=0)
    end = torch.clip(center + half_width, max=n_bins)
    return center[:, 0].numpy(), ((center >= 1) & (idx >= start) & (idx < end)).numpy()


def kth_harmonic(k, harmonic_part, f0, hop_size, win_size, samplerate, half_width=3.5):
    """The dense form: torch.stft -> mask -> torch.istft, in harmonic_part's dtype."""
    wav = torch.from_numpy(np.ascontiguousarray(harmonic_part))[None]
    n = wav.shape[1]
    _, mask = kth_mask(k, np.asarray(f0, harmonic_part.dtype), n, hop_size, win_size, samplerate, half_width)
    mask = torch.from_numpy(mask)[None]
    window = nuttall(win_size, wav.dtype)
    spec = torch.stft(wav, n_fft=win_size, win_length=win_size, hop_length=hop_size, window=window, center=True,
                      return_complex=True).permute(0, 2, 1)
    T = spec.shape[1]
    if mask.shape[1] < T:
        mask = F.pad(mask, [0, 0, 0, T - mask.shape[1]])
    spec = spec * mask[:, :T]
    return torch.istft(spec.permute(0, 2, 1), n_fft=win_size, win_length=win_size, hop_length=hop_size, window=window,
                       center=True, length=n)[0].numpy()


def kth_bins(k, f0, n_samples, hop_size, win_size, samplerate, half_width=3.5):
    """(first kept bin, count) per frame, from the float32 mask arithmetic: what the f0 kernel emits."""
    _, mask = kth_mask(k, np.asarray(f0, np.float32), n_samples, hop_size, win_size, samplerate, half_width)
    T = n_samples // hop_size + 1
    mask = mask[:T]
    return mask.argmax(axis=1) * mask.any(axis=1), mask.sum(axis=1)


def kth_harmonic_sparse(k, harmonic_part, f0, hop_size, win_size, samplerate, half_width=3.5):
    """The sparse form in float64: per frame the kept bins' DFT sums of the reflect-padded, windowed frame; per
    sample the sum over the covering frames of w[m] * (Re(X) cos / N at DC and Nyquist, 2 Re(X e^{+2 pi i b m / N}) / N
    elsewhere), divided by the squared-window envelope of the frames that exist."""
    x = np.asarray(harmonic_part, np.float64)
    n, win, hop = len(x), win_size, hop_size
    first, count = kth_bins(k, f0, n, hop, win, samplerate, half_width)
    w = nuttall(win, torch.float64).numpy()
    xp = np.pad(x, win // 2, mode="reflect")
    T = n // hop + 1
    m = np.arange(win)
    acc, env = np.zeros(len(xp)), np.zeros(len(xp))
    for t in range(T):
        env[t * hop:t * hop + win] += w * w
        fr = xp[t * hop:t * hop + win] * w
        for b in range(first[t], first[t] + count[t]):
            ang = 2 * np.pi * ((b * m) % win) / win
            X = np.sum(fr * np.exp(-1j * ang))
            seg = X.real * np.cos(ang) / win if b in (0, win // 2) else 2 * (X * np.exp(1j * ang)).real / win
            acc[t * hop:t * hop + win] += w * seg
    return acc[win // 2:win // 2 + n] / env[win // 2:win // 2 + n]


def tension_from(energy_full, energy_base, domain):
    """binarizer_utils.py:202-210 on two amplitude curves, in their dtype."""
    one = energy_full.dtype.type
    t = np.sqrt(np.clip(energy_full ** 2 - energy_base ** 2, a_min=0, a_max=None)) / (energy_full + one(1e-5))
    if domain == "ratio":
        return np.clip(t, a_min=0, a_max=1)
    if domain == "db":
        return amplitude_to_db(np.clip(t, a_min=one(1e-5), a_max=1))
    if domain == "logit":
        t = np.clip(t, a_min=one(1e-4), a_max=one(1 - 1e-4))
        return np.log(t / (1 - t))
    raise ValueError(f"Unknown domain: {domain}")


def get_tension(sp, mel_len, f0, hop_size, win_size, samplerate, kernel_size, half_width=3.5, domain="logit",
                pad_mode="reflect", base=None):
    base = kth_harmonic(0, sp, f0, hop_size, win_size, samplerate, half_width) if base is None else base
    ef = get_energy(sp, mel_len, hop_size, win_size, "amplitude", pad_mode)
    eb = get_energy(base.astype(sp.dtype), mel_len, hop_size, win_size, "amplitude", pad_mode)
    return smooth(tension_from(ef, eb, domain), kernel_size)
