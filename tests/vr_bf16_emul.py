"""CPU emulation of the separation's bf16 conv mode (PD_VR_OPT_CONV_DTYPE = PD_DTYPE_BF16, include/prodiff_hip.h),
written from the formulas with torch's functional ops as tests/vr_ref.py is, and with none of the reference's modules.

What the mode does, restated:
  * every BatchNorm is folded into its conv in double, w' = w g / sqrt(var + 1e-5), and the result rounded once to
    f32 (the create's packed tile), then once more to bf16 (the mirror); the bias beta - mean g / sqrt(var + 1e-5)
    is rounded to f32 and stays f32;
  * before every conv except `out`, the input (an f32 map, after the bilinear x2 and the concatenation) is rounded to
    bf16, nearest even; the border's zeros are exact either way;
  * products of two bf16 values are exact in f32, the sums are taken in f32 on the GPU and in double here: the two
    differ only in summation order, and in the rare bf16 rounding of a later layer's input that this flips;
  * the stored maps are f32: every conv's output is rounded to f32 after bias and activation;
  * the LSTM, its two Linear layers, the frequency mean, `out`, the bounded mask and the transforms are those of
    vr_ref, in double.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from prodiff_amd.vr import padded_frames
from tests import vr_ref as R


def _f32(x):
    return x.float().double()


def _bf16(x):
    """double -> f32 -> bf16 (nearest even both times) -> double."""
    return x.float().bfloat16().double()


def folded(P, p):
    """(bf16-rounded folded weight, f32-rounded folded bias) of conv + BatchNorm `p`, as doubles."""
    w = R._t(P, p + ".conv.0.weight")
    scale = R._t(P, p + ".conv.1.weight") / torch.sqrt(R._t(P, p + ".conv.1.running_var") + 1e-5)
    bias = R._t(P, p + ".conv.1.bias") - R._t(P, p + ".conv.1.running_mean") * scale
    return _bf16(_f32(w * scale[:, None, None, None])), _f32(bias)


def conv(x, w, b, stride, pad, dil, order=None):
    """The conv of bf16-valued x and w: the exact products summed in double, or (``order``: a torch.Generator) in f32
    over a random permutation of the input channels -- another summation order of the same sum, as the GPU's is."""
    if order is None:
        return F.conv2d(x, w, b, stride, pad, dil)
    perm = torch.randperm(x.shape[1], generator=order)
    return F.conv2d(x.float()[:, perm].contiguous(), w.float()[:, perm].contiguous(), b.float(), stride, pad, dil).double()


def cba(P, p, x, stride=1, pad=0, dil=1, act="relu", order=None):
    w, b = folded(P, p)
    y = conv(_bf16(x), w, b, stride, pad, dil, order)
    return _f32(F.relu(y) if act == "relu" else F.leaky_relu(y, 0.01))


def lstm_module(P, p, x, order=None):
    N, _, nbins, nframes = x.shape
    h = cba(P, p + ".conv", x, order=order)[:, 0].permute(2, 0, 1)
    h = torch.cat([R.lstm_dir(P, p + ".lstm", "", h), R.lstm_dir(P, p + ".lstm", "_reverse", h)], dim=-1)
    h = h.reshape(-1, h.shape[-1]) @ R._t(P, p + ".dense.0.weight").T + R._t(P, p + ".dense.0.bias")
    h = F.batch_norm(h, R._t(P, p + ".dense.1.running_mean"), R._t(P, p + ".dense.1.running_var"),
                     R._t(P, p + ".dense.1.weight"), R._t(P, p + ".dense.1.bias"), False, 0.0, 1e-5)
    return F.relu(h).reshape(nframes, N, 1, nbins).permute(1, 2, 3, 0)


def decoder(P, p, x, skip, order=None):
    x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
    assert x.shape[2:] == skip.shape[2:]
    return cba(P, p + ".conv1", torch.cat([x, skip], dim=1), 1, 1, order=order)


def base_net(P, p, x, order=None):
    e = [cba(P, p + ".enc1", x, 1, 1, order=order)]
    for i in (2, 3, 4, 5):
        h = cba(P, f"{p}.enc{i}.conv1", e[-1], 2, 1, act="leaky", order=order)
        e.append(cba(P, f"{p}.enc{i}.conv2", h, 1, 1, act="leaky", order=order))
    e5 = e[4]
    feats = [cba(P, p + ".aspp.conv1.1", _f32(e5.mean(-2, keepdim=True)), order=order).repeat(1, 1, e5.shape[2], 1),
             cba(P, p + ".aspp.conv2", e5, order=order)]
    for i, d in zip((3, 4, 5), ((4, 2), (8, 4), (12, 6))):
        feats.append(cba(P, f"{p}.aspp.conv{i}", e5, 1, d, d, order=order))
    h = cba(P, p + ".aspp.bottleneck", torch.cat(feats, dim=1), order=order)
    h = decoder(P, p + ".dec4", h, e[3], order)
    h = decoder(P, p + ".dec3", h, e[2], order)
    h = decoder(P, p + ".dec2", h, e[1], order)
    h = torch.cat([h, _f32(lstm_module(P, p + ".lstm_dec2", h, order))], dim=1)
    return decoder(P, p + ".dec1", h, e[0], order)


def mask(P, spec, order=None):
    """spec complex [B, C, n_fft/2 + 1, T] -> the bounded complex mask of the bf16 mode, same shape, float64.
    ``order``: a torch.Generator -- the convs sum in f32 over freshly permuted input channels (``conv``)."""
    spec = torch.as_tensor(spec).to(torch.complex128)
    C = spec.shape[1]
    x = torch.cat([spec.real, spec.imag], dim=1)[:, :, :spec.shape[2] - 1]
    bw = x.shape[2] // 2
    lo, hi = x[:, :, :bw], x[:, :, bw:]
    l1 = cba(P, "stg1_low_band_net.1", base_net(P, "stg1_low_band_net.0", lo, order), order=order)
    h1 = base_net(P, "stg1_high_band_net", hi, order)
    aux1 = torch.cat([l1, h1], dim=2)
    l2 = cba(P, "stg2_low_band_net.1", base_net(P, "stg2_low_band_net.0", torch.cat([lo, l1], dim=1), order),
             order=order)
    h2 = base_net(P, "stg2_high_band_net", torch.cat([hi, h1], dim=1), order)
    aux2 = torch.cat([l2, h2], dim=2)
    f3 = base_net(P, "stg3_full_band_net", torch.cat([x, aux1, aux2], dim=1), order)
    m = F.conv2d(f3, R._t(P, "out.weight"))                  # `out` stays fp32: unrounded input and weights
    m = torch.complex(m[:, :C], m[:, C:])
    mag = m.abs()
    m = torch.tanh(mag) * m / (mag + 1e-8)
    return torch.cat([m, m[:, :, -1:]], dim=2)


def predict_from_spec(P, spec, n_fft, hop, L):
    """The fixture's spectrum [B, C, n_fft/2 + 1, T] of L samples -> (mask, harmonic y) of the bf16 mode, float64; the
    inverse transform is vr_ref's float64 one."""
    s = torch.as_tensor(spec).to(torch.complex128)
    m = mask(P, s)
    return m.numpy(), R.istft(s * m, n_fft, hop, padded_frames(L, hop)[1], L).numpy()


# ---------------------------------------------------------------- shared by the CPU and the GPU tests
# The mask's largest absolute error (bf16 mode against the fixture's f32 mask) has no project bar.  MASK_MAX_GPU is the
# largest value the native mode measured over the five cases of tests/vr_cases.py on an MI355X (the per-case values
# are in tests/test_vr_bf16_cpu.py's docstring and DESIGN.md §14); the bar is twice that: the emulation's own values
# spread by about 5x across the five fixtures, the factor covers a fixture's spread around the worst one.
MASK_MAX_GPU = 3.037e-2
MASK_MAX_BAR = 2 * MASK_MAX_GPU


def pairs(z):
    """complex [...] -> float64 [..., 2]: norms and peaks over a complex array's real and imaginary parts."""
    z = np.asarray(z)
    return np.stack([z.real, z.imag], axis=-1).astype(np.float64)


@functools.lru_cache(maxsize=None)
def emulated(name):
    """(mask, y) of the emulation on the fixture's spectrum, computed once per session and not to be written to."""
    from tests import golden_io
    from tests import vr_cases as VC
    n_fft, hop = VC.CASES[name][:2]
    m, y = predict_from_spec(VC.case_params(name), golden_io.load(name)["spec"], n_fft, hop, VC.CASES[name][6])
    m.setflags(write=False)
    y.setflags(write=False)
    return m, y


ORDER_DRAWS = {True: 4, False: 2}      # f32 summation orders drawn per case: small nets, full-size nets
ORDER_FACTOR = 1.5


@functools.lru_cache(maxsize=None)
def order_noise(name):
    """What the f32 summation order alone is worth on this case: the largest rel-L2 distance, over ORDER_DRAWS seeded
    channel permutations, between the emulated mask with its convs summed in f32 and the one summed in double."""
    from tests import golden_io
    from tests import vr_cases as VC
    exact = pairs(emulated(name)[0])
    spec, P = golden_io.load(name)["spec"], VC.case_params(name)
    out = []
    for seed in range(ORDER_DRAWS[name in VC.SMALL]):
        m = mask(P, spec, torch.Generator().manual_seed(seed)).numpy()
        out.append(float(np.linalg.norm(pairs(m) - exact) / np.linalg.norm(exact)))
    return max(out)
