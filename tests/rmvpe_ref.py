"""float64 restatements for the RMVPE tests, written from the formulas (include/prodiff_hip.h, "pitch extraction"),
independent of the native code and of the reference's modules: the E2E0 network, to_local_average_f0, the
centred mel front end (torch.stft(center=True) in float64) and the HTK mel filterbank.  tests/test_rmvpe_cpu.py
pins the network to the fixtures' float64 tensors.
"""
import numpy as np

from tests import rmvpe_cases as RC

EPS = 1e-5


# ---------------------------------------------------------------- network
def _bn(P, p, x):
    """eval BatchNorm over the last (channel) axis"""
    g, b, m, v = (P[f"{p}.{k}"].astype(np.float64) for k in ("weight", "bias", "running_mean", "running_var"))
    return (x - m) / np.sqrt(v + EPS) * g + b


def _conv(x, w, pad):
    """x [B, H, W, Ci], w [Co, Ci, kh, kw] (Conv2d layout), stride 1, zero padding ``pad`` -> [B, H, W, Co]"""
    w = w.astype(np.float64)
    Co, Ci, kh, kw = w.shape
    B, H, W, _ = x.shape
    xp = np.pad(x, ((0, 0), (pad, pad), (pad, pad), (0, 0)))
    cols = np.concatenate([xp[:, dy:dy + H, dx:dx + W, :] for dy in range(kh) for dx in range(kw)], axis=-1)
    wm = w.transpose(2, 3, 1, 0).reshape(kh * kw * Ci, Co)      # rows ordered tap, then input channel
    return (cols.reshape(-1, kh * kw * Ci) @ wm).reshape(B, H, W, Co)


def _conv_transpose(x, w):
    """ConvTranspose2d(3x3, stride 2, padding 1, output_padding 1, no bias): x [B, H, W, Ci], w [Ci, Co, 3, 3]
    -> [B, 2H, 2W, Co], scattered: input pixel (i, j) adds x w[ky][kx] at output (2i - 1 + ky, 2j - 1 + kx)."""
    w = w.astype(np.float64)
    B, H, W, Ci = x.shape
    Co = w.shape[1]
    full = np.zeros((B, 2 * H + 2, 2 * W + 2, Co))          # output index + 1
    for ky in range(3):
        for kx in range(3):
            full[:, ky:ky + 2 * H:2, kx:kx + 2 * W:2, :] += x @ w[:, :, ky, kx]
    return full[:, 1:2 * H + 1, 1:2 * W + 1, :]


def _block(P, p, x):
    h = np.maximum(_bn(P, p + ".conv.1", _conv(x, P[p + ".conv.0.weight"], 1)), 0.0)
    h = np.maximum(_bn(P, p + ".conv.4", _conv(h, P[p + ".conv.3.weight"], 1)), 0.0)
    if p + ".shortcut.weight" in P:
        return h + _conv(x, P[p + ".shortcut.weight"], 0) + P[p + ".shortcut.bias"].astype(np.float64)
    return h + x


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def _gru_direction(P, suffix, x, reverse):
    """x [B, T, I] -> [B, T, H]; gates r, z, n"""
    Wi, Wh, bi, bh = (P[f"fc.0.gru.{k}_l0{suffix}"].astype(np.float64)
                      for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
    H = Wh.shape[1]
    B, T, _ = x.shape
    xp = x @ Wi.T + bi
    h = np.zeros((B, H))
    out = np.zeros((B, T, H))
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        hp = h @ Wh.T + bh
        r = _sigmoid(xp[:, t, :H] + hp[:, :H])
        z = _sigmoid(xp[:, t, H:2 * H] + hp[:, H:2 * H])
        n = np.tanh(xp[:, t, 2 * H:] + r * hp[:, 2 * H:])
        h = (1.0 - z) * n + z * h
        out[:, t] = h
    return out


def e2e0(P, model, mel):
    """mel [B, n_mels, T] -> (feat [B, T, 3 n_mels], hidden [B, T, n_class]) in float64"""
    L, nb = model["en_de_layers"], model["n_blocks"]
    x = np.asarray(mel, np.float64).transpose(0, 2, 1)[..., None]        # [B, T, F, 1]
    x = _bn(P, "unet.encoder.bn", x)
    skips = []
    for i in range(L):
        for j in range(nb):
            x = _block(P, f"unet.encoder.layers.{i}.conv.{j}", x)
        skips.append(x)
        B, H, W, C = x.shape
        x = x.reshape(B, H // 2, 2, W // 2, 2, C).mean(axis=(2, 4))
    for i in range(model["inter_layers"]):
        for j in range(nb):
            x = _block(P, f"unet.intermediate.layers.{i}.conv.{j}", x)
    for i in range(L):
        p = f"unet.decoder.layers.{i}"
        x = np.maximum(_bn(P, p + ".conv1.1", _conv_transpose(x, P[p + ".conv1.0.weight"])), 0.0)
        x = np.concatenate([x, skips[L - 1 - i]], axis=-1)
        for j in range(nb):
            x = _block(P, f"{p}.conv2.{j}", x)
    x = _conv(x, P["cnn.weight"], 1) + P["cnn.bias"].astype(np.float64)   # [B, T, F, 3]
    B, T, F, _ = x.shape
    feat = x.transpose(0, 1, 3, 2).reshape(B, T, 3 * F)
    if model["n_gru"]:
        g = np.concatenate([_gru_direction(P, "", feat, False), _gru_direction(P, "_reverse", feat, True)], axis=-1)
        logits = g @ P["fc.1.weight"].astype(np.float64).T + P["fc.1.bias"].astype(np.float64)
    else:
        logits = feat @ P["fc.0.weight"].astype(np.float64).T + P["fc.0.bias"].astype(np.float64)
    return feat, _sigmoid(logits)


# ---------------------------------------------------------------- decode
def local_average_f0(hidden, thred, center=None, const=RC.CONST):
    """hidden [..., n_class] -> f0 [...] (float64); ``thred`` is compared as the float32 the kernel receives."""
    h = np.asarray(hidden, np.float64)
    n = h.shape[-1]
    c = np.argmax(h, axis=-1) if center is None else np.clip(np.asarray(center, np.int64), 0, n - 1)
    idx = np.arange(n)
    mask = (idx >= np.maximum(c - 4, 0)[..., None]) & (idx < np.minimum(c + 5, n)[..., None])
    wgt = h * mask
    den = wgt.sum(-1)
    cents = (wgt * (20.0 * idx + const)).sum(-1) / (den + (den == 0))
    f0 = 10.0 * 2.0 ** (cents / 1200.0)
    return np.where(h.max(-1) < np.float64(np.float32(thred)), 0.0, f0)


def decode_cases():
    """Hand-built salience [8, 360], one frame of each kind: peaks at bins 0, 3, 356 and 359 (window clipping),
    an all-zero frame, a frame whose maximum is below 0.03, an exact tie (lowest index wins), an ordinary frame."""
    n = RC.N_CLASS
    rng = np.random.default_rng(11)
    h = (0.01 * rng.random((8, n))).astype(np.float32)
    for row, peak in enumerate((0, 3, 356, 359)):
        for i in range(max(peak - 6, 0), min(peak + 7, n)):
            h[row, i] = 0.9 * np.exp(-0.5 * ((i - peak) / 2.0) ** 2)
    h[4] = 0.0
    h[5] *= 0.5                   # maximum < 0.005
    h[6, 100] = h[6, 200] = 0.75  # tie
    h[6, 96:105] += 0.125
    h[6, 200] = h[6, 100]
    h[7, 180:189] = np.float32([0.1, 0.2, 0.4, 0.7, 0.95, 0.6, 0.3, 0.2, 0.1])
    return h


# ---------------------------------------------------------------- filterbank and centred mel
def htk_filterbank(sr, n_fft, n_mels, fmin, fmax):
    """float64 [n_mels, n_fft // 2 + 1]: triangles between n_mels + 2 points equally spaced on the HTK scale
    mel = 2595 log10(1 + f / 700), each scaled by 2 / (its base in Hz)."""
    def to_mel(f):
        return 2595.0 * np.log10(1.0 + f / 700.0)
    fmax = sr / 2.0 if fmax is None else float(fmax)
    pts = 700.0 * (10.0 ** (np.linspace(to_mel(float(fmin)), to_mel(fmax), n_mels + 2) / 2595.0) - 1.0)
    freqs = np.arange(1 + n_fft // 2) * (sr / n_fft)
    out = np.zeros((n_mels, freqs.size))
    for m in range(n_mels):
        lo, mid, hi = pts[m], pts[m + 1], pts[m + 2]
        tri = np.minimum((freqs - lo) / (mid - lo), (hi - freqs) / (hi - mid))
        out[m] = np.maximum(tri, 0.0) * 2.0 / (hi - lo)
    return out


def centered_mel(wav, basis, n_fft=1024, hop=160, clamp=1e-5):
    """modules/rmvpe/spec.py with keyshift 0: wav [B, L] -> (spec [B, T, n_fft/2 + 1], mel linear [B, T, n_mels],
    log-mel [B, T, n_mels]) in float64, T = 1 + L // hop."""
    import torch
    y = torch.from_numpy(np.asarray(wav, np.float64))
    win = torch.hann_window(n_fft, dtype=torch.float64)
    spec = torch.stft(y, n_fft, hop_length=hop, win_length=n_fft, window=win, center=True, pad_mode="reflect",
                      return_complex=True).abs().numpy().transpose(0, 2, 1)
    lin = spec @ np.asarray(basis, np.float64).T
    return spec, lin, np.log(np.maximum(lin, clamp))
