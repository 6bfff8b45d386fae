"""float64 restatement of the harmonic-noise separation for the tests, written from the formulas
(include/prodiff_hip.h, "harmonic-noise separation") with torch's functional ops and none of the reference's
modules.  tests/test_vr_cpu.py pins it to the reference's own float64 run."""
import numpy as np
import torch
import torch.nn.functional as F

from prodiff_amd.vr import padded_frames


def _t(P, k):
    return torch.from_numpy(np.asarray(P[k])).double()


def cba(P, p, x, stride=1, pad=0, dil=1, act="relu"):
    y = F.conv2d(x, _t(P, p + ".conv.0.weight"), None, stride, pad, dil)
    y = F.batch_norm(y, _t(P, p + ".conv.1.running_mean"), _t(P, p + ".conv.1.running_var"),
                     _t(P, p + ".conv.1.weight"), _t(P, p + ".conv.1.bias"), False, 0.0, 1e-5)
    return F.relu(y) if act == "relu" else F.leaky_relu(y, 0.01)


def lstm_dir(P, p, suffix, x):
    """x [T, N, K] -> h [T, N, H]; gate order i, f, g, o."""
    wih, whh = _t(P, f"{p}.weight_ih_l0{suffix}"), _t(P, f"{p}.weight_hh_l0{suffix}")
    b = _t(P, f"{p}.bias_ih_l0{suffix}") + _t(P, f"{p}.bias_hh_l0{suffix}")
    H = whh.shape[1]
    h = torch.zeros(x.shape[1], H, dtype=torch.float64)
    c = torch.zeros_like(h)
    out = [None] * x.shape[0]
    order = range(x.shape[0] - 1, -1, -1) if suffix else range(x.shape[0])
    for t in order:
        g = x[t] @ wih.T + h @ whh.T + b
        i, f, gg, o = g[:, :H], g[:, H:2 * H], g[:, 2 * H:3 * H], g[:, 3 * H:]
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
        h = torch.sigmoid(o) * torch.tanh(c)
        out[t] = h
    return torch.stack(out)


def lstm_module(P, p, x):
    N, _, nbins, nframes = x.shape
    h = cba(P, p + ".conv", x)[:, 0].permute(2, 0, 1)
    h = torch.cat([lstm_dir(P, p + ".lstm", "", h), lstm_dir(P, p + ".lstm", "_reverse", h)], dim=-1)
    h = h.reshape(-1, h.shape[-1]) @ _t(P, p + ".dense.0.weight").T + _t(P, p + ".dense.0.bias")
    h = F.batch_norm(h, _t(P, p + ".dense.1.running_mean"), _t(P, p + ".dense.1.running_var"),
                     _t(P, p + ".dense.1.weight"), _t(P, p + ".dense.1.bias"), False, 0.0, 1e-5)
    return F.relu(h).reshape(nframes, N, 1, nbins).permute(1, 2, 3, 0)


def decoder(P, p, x, skip):
    x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
    assert x.shape[2:] == skip.shape[2:]        # crop_center is the identity
    return cba(P, p + ".conv1", torch.cat([x, skip], dim=1), 1, 1)


def base_net(P, p, x):
    e = [cba(P, p + ".enc1", x, 1, 1)]
    for i in (2, 3, 4, 5):
        h = cba(P, f"{p}.enc{i}.conv1", e[-1], 2, 1, act="leaky")
        e.append(cba(P, f"{p}.enc{i}.conv2", h, 1, 1, act="leaky"))
    e5 = e[4]
    feats = [cba(P, p + ".aspp.conv1.1", e5.mean(-2, keepdim=True)).repeat(1, 1, e5.shape[2], 1),
             cba(P, p + ".aspp.conv2", e5)]
    for i, d in zip((3, 4, 5), ((4, 2), (8, 4), (12, 6))):
        feats.append(cba(P, f"{p}.aspp.conv{i}", e5, 1, d, d))
    h = cba(P, p + ".aspp.bottleneck", torch.cat(feats, dim=1))
    h = decoder(P, p + ".dec4", h, e[3])
    h = decoder(P, p + ".dec3", h, e[2])
    h = decoder(P, p + ".dec2", h, e[1])
    h = torch.cat([h, lstm_module(P, p + ".lstm_dec2", h)], dim=1)
    return decoder(P, p + ".dec1", h, e[0])


def mask(P, spec):
    """spec complex [B, C, n_fft/2 + 1, T] -> the bounded complex mask of the same shape, float64."""
    spec = torch.as_tensor(spec).to(torch.complex128)
    C = spec.shape[1]
    x = torch.cat([spec.real, spec.imag], dim=1)[:, :, :spec.shape[2] - 1]
    bw = x.shape[2] // 2
    lo, hi = x[:, :, :bw], x[:, :, bw:]
    l1 = cba(P, "stg1_low_band_net.1", base_net(P, "stg1_low_band_net.0", lo))
    h1 = base_net(P, "stg1_high_band_net", hi)
    aux1 = torch.cat([l1, h1], dim=2)
    l2 = cba(P, "stg2_low_band_net.1", base_net(P, "stg2_low_band_net.0", torch.cat([lo, l1], dim=1)))
    h2 = base_net(P, "stg2_high_band_net", torch.cat([hi, h1], dim=1))
    aux2 = torch.cat([l2, h2], dim=2)
    f3 = base_net(P, "stg3_full_band_net", torch.cat([x, aux1, aux2], dim=1))
    m = F.conv2d(f3, _t(P, "out.weight"))
    m = torch.complex(m[:, :C], m[:, C:])
    mag = m.abs()
    m = torch.tanh(mag) * m / (mag + 1e-8)
    return torch.cat([m, m[:, :, -1:]], dim=2)


def window64(n_fft):
    """The reference's window in its float64 run: the float32 ``window`` buffer cast by ``.double()``."""
    return torch.hann_window(n_fft).double()


def stft(wav, n_fft, hop):
    """predict_from_audio's front end: [B, C, L] -> (complex [B, C, n_fft/2 + 1, T], Tl_pad), float64."""
    x = torch.as_tensor(wav).double()
    B, C, L = x.shape
    T, Tl_pad, T_pad = padded_frames(L, hop)
    x = F.pad(x.reshape(B * C, L), (Tl_pad, T_pad - Tl_pad))
    s = torch.stft(x, n_fft, hop, window=window64(n_fft), return_complex=True,
                   pad_mode="constant")
    assert s.shape[-1] == T
    return s.reshape(B, C, s.shape[-2], T), Tl_pad


def istft(spec, n_fft, hop, Tl_pad, L):
    spec = torch.as_tensor(spec).to(torch.complex128)
    B, C = spec.shape[:2]
    y = torch.istft(spec.reshape(B * C, *spec.shape[2:]), n_fft, hop, window=window64(n_fft))
    return y[:, Tl_pad:Tl_pad + L].reshape(B, C, L)


def predict_from_audio(P, wav, n_fft, hop):
    s, Tl_pad = stft(wav, n_fft, hop)
    m = mask(P, s)
    return m.numpy(), istft(s * m, n_fft, hop, Tl_pad, wav.shape[-1]).numpy()


def istft_tables(n_fft, hop):
    """The inverse as one matrix product over hop-sized segments (float64): (table [R, 2, n_fft/2 + 1, hop],
    window): segment j of the overlap-add = sum_q re(j - q) @ table[q, 0] + im(j - q) @ table[q, 1]."""
    R, nb = n_fft // hop, n_fft // 2 + 1
    n = np.arange(n_fft)
    w = 0.5 - 0.5 * np.cos(2 * np.pi * n / n_fft)
    k = np.arange(nb)[:, None]
    ph = 2 * np.pi * ((n[None, :] * k) % n_fft) / n_fft
    ck = np.where((k == 0) | (2 * k == n_fft), 1.0, 2.0)
    tc = w * ck * np.cos(ph) / n_fft
    ts = -w * ck * np.sin(ph) / n_fft
    ts[0] = 0.0
    ts[-1] = 0.0
    tab = np.stack([tc, ts]).reshape(2, nb, R, hop).transpose(2, 0, 1, 3)
    return tab, w


def istft_by_segments(spec, n_fft, hop, lead, L_out):
    """The samples [lead - n_fft/2, .. + L_out) of torch.istft(spec) by the segment product; spec complex [T, nb]
    frames-major, float64."""
    tab, w = istft_tables(n_fft, hop)
    T = spec.shape[0]
    R = n_fft // hop
    nseg = T + R - 1
    ola = np.zeros((nseg, hop))
    env = np.zeros((nseg, hop))
    for q in range(R):
        ola[q:q + T] += spec.real @ tab[q, 0] + spec.imag @ tab[q, 1]
        env[q:q + T] += (w[q * hop:(q + 1) * hop] ** 2)[None, :]
    y = (ola / np.maximum(env, 1e-30)).reshape(-1)
    return y[lead:lead + L_out]
