"""CPU emulation of the pitch extractor's bf16 modes (pd_rmvpe_set_option, include/prodiff_hip.h), written from the
formulas in float64 on tests/rmvpe_ref.py's helpers and independent of the native code.

What the modes do, restated:
  PD_RMVPE_OPT_CONV_DTYPE = bf16
    * every BatchNorm behind a 3x3 conv (and behind a decoder's transposed conv) is folded into it in double,
      w' = w g / sqrt(var + 1e-5), the result rounded once to f32 (the create's packed tile) and once more to bf16
      (the mirror); the bias beta - mean g / sqrt(var + 1e-5) is rounded to f32 and stays f32; a block's 1x1 shortcut
      has no BatchNorm: its f32 weights are rounded to bf16, its bias stays f32;
    * the input of every such conv (an f32 map; for a decoder's first block the concatenation of two) is rounded to
      bf16, nearest even; the border's and the transposed conv's stuffed zeros are exact either way;
    * products of two bf16 values are exact in f32; the sums are taken in f32 on the GPU and in double here, so the
      two differ in summation order, and in the rare bf16 rounding of a later layer's input that this flips;
    * the stored maps are f32: every conv's output is rounded to f32 after bias, ReLU and the residual add;
    * the first conv (C_in = 1, with encoder.bn) and its shortcut, the pools and `cnn` are those of rmvpe_ref, in
      double on unrounded operands.
  PD_RMVPE_OPT_GRU_DTYPE = bf16
    * hp = bf16(h_{t-1}) bf16(W_hh)^T + b_hh; the gates and h = (1 - z) n + z h_{t-1} take the unrounded h_{t-1};
      the carried state and the output are f32.  W_ih x + b_ih, the head and the sigmoid are rmvpe_ref's, in double.

``order`` (a numpy Generator) states the other arithmetic, the GPU's: every bf16 product sum is taken in f32 over a
freshly drawn permutation of the input channels (of the hidden units, for the recurrence), and what feeds a bf16
rounding from the fp32 side -- encoder.bn, the first conv and its shortcut, and the 2x2 pools -- is evaluated in
f32 as conv_in_kernel and avgpool_kernel state it (_first_block_f32, _pool).  order_noise is what that alone is worth on a case; tests/test_gpu_vr_bf16.py's header has
the construction and its reasons.  The fp32 side belongs to it: on rmvpe_shallow (nine convs deep) the first MI355X
run sat 1.45e-4 (feat) from this emulation with four draws of the bf16 sums alone at 2.8e-5; with nothing changed but
the first conv and the pools computed in f32, the way conv_in_kernel and avgpool_kernel do, a CPU restatement of the
kernel's own summation order was 6.3e-6 from the native result, and 1.45e-4 from the double-summed emulation: an f32
rounding of the first conv's output flips the bf16 rounding of the second conv's input as a summation order does.
"""
import functools

import numpy as np
import torch

from tests import rmvpe_cases as RC
from tests import rmvpe_ref as R


def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def _bf16(x):
    """double -> f32 -> bf16 (nearest even both times) -> double"""
    return torch.from_numpy(np.ascontiguousarray(x, np.float64)).float().bfloat16().double().numpy()


def _scale_bias(P, bn):
    g, b, m, v = (P[f"{bn}.{k}"].astype(np.float64) for k in ("weight", "bias", "running_mean", "running_var"))
    s = g / np.sqrt(v + R.EPS)
    return s, _f32(b - m * s)


def folded(P, conv_key, bn, transposed=False):
    """(bf16-rounded folded weight in its stored layout, f32-rounded folded bias) of a conv and the BatchNorm behind
    it, as doubles; ``transposed``: ConvTranspose2d's [Ci, Co, 3, 3]."""
    s, bias = _scale_bias(P, bn)
    w = P[conv_key].astype(np.float64)
    w = w * (s[None, :, None, None] if transposed else s[:, None, None, None])
    return _bf16(_f32(w)), bias


def _matmul(a, b, group, order):
    """a [M, K] @ b [K, N], K = taps x ``group`` channels: in double, or (``order``) in f32 with the channels of
    every tap permuted -- another summation order of the same sum, as the GPU's is."""
    if order is None:
        return a @ b
    perm = order.permutation(group)
    idx = (np.arange(a.shape[1] // group)[:, None] * group + perm[None, :]).reshape(-1)
    return (np.ascontiguousarray(a[:, idx], np.float32) @ np.ascontiguousarray(b[idx], np.float32)).astype(np.float64)


def _conv(x, w, pad, order=None):
    """rmvpe_ref._conv of values that are already rounded: x [B, H, W, Ci], w [Co, Ci, kh, kw] -> [B, H, W, Co]"""
    Co, Ci, kh, kw = w.shape
    B, H, W, _ = x.shape
    xp = np.pad(x, ((0, 0), (pad, pad), (pad, pad), (0, 0)))
    cols = np.concatenate([xp[:, dy:dy + H, dx:dx + W, :] for dy in range(kh) for dx in range(kw)], axis=-1)
    wm = w.transpose(2, 3, 1, 0).reshape(kh * kw * Ci, Co)
    return _matmul(cols.reshape(-1, kh * kw * Ci), wm, Ci, order).reshape(B, H, W, Co)


def _conv_transpose(x, w, order=None):
    """rmvpe_ref._conv_transpose of rounded values; with ``order`` the taps add up in f32"""
    B, H, W, Ci = x.shape
    Co = w.shape[1]
    full = np.zeros((B, 2 * H + 2, 2 * W + 2, Co), np.float64 if order is None else np.float32)
    flat = x.reshape(-1, Ci)
    for ky in range(3):
        for kx in range(3):
            full[:, ky:ky + 2 * H:2, kx:kx + 2 * W:2, :] += _matmul(flat, w[:, :, ky, kx], Ci, order).reshape(B, H, W, Co)
    return full[:, 1:2 * H + 1, 1:2 * W + 1, :].astype(np.float64)


def _block(P, p, x, order=None):
    """ConvBlockRes in the bf16 conv mode; the network's first block (C_in = 1) keeps its first conv and its shortcut
    in double, as the VALU kernel that runs them is fp32."""
    first = x.shape[-1] == 1
    if first:
        h = np.maximum(R._bn(P, p + ".conv.1", R._conv(x, P[p + ".conv.0.weight"], 1)), 0.0)
    else:
        w, b = folded(P, p + ".conv.0.weight", p + ".conv.1")
        h = np.maximum(_conv(_bf16(x), w, 1, order) + b, 0.0)
    w, b = folded(P, p + ".conv.3.weight", p + ".conv.4")
    h = np.maximum(_conv(_bf16(_f32(h)), w, 1, order) + b, 0.0)
    if p + ".shortcut.weight" not in P:
        return _f32(h + x)
    bs = P[p + ".shortcut.bias"].astype(np.float64)
    if first:
        sc = R._conv(x, P[p + ".shortcut.weight"], 0) + bs
    else:
        sc = _conv(_bf16(x), _bf16(P[p + ".shortcut.weight"].astype(np.float64)), 0, order) + bs
    return _f32(h + _f32(sc))


def _first_block_f32(P, p, raw, order):
    """_block for the network's first block, from the raw input [B, H, W, 1], with its fp32 side in f32 as
    conv_in_kernel states it: encoder.bn as one fma with f32 scale and shift, the folded first conv as an fma chain
    over its nine taps with f32 weights and bias, the shortcut as one fma; then the second conv (bf16, ``order``)."""
    def fma(a, b, c):       # exact in double up to a double rounding far below f32's
        return _f32(_f32(a) * _f32(b) + _f32(c))
    g, beta, mean, var = (P[f"unet.encoder.bn.{k}"].astype(np.float64) for k in ("weight", "bias", "running_mean", "running_var"))
    s0 = g[0] / np.sqrt(var[0] + R.EPS)
    x = fma(raw[..., 0], s0, beta[0] - mean[0] * s0)                    # [B, H, W]
    B, H, W = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1)))
    s, b1 = _scale_bias(P, p + ".conv.1")
    w1 = _f32(P[p + ".conv.0.weight"].astype(np.float64).reshape(-1, 9) * s[:, None])       # [Co, 9]
    acc = np.zeros((B, H, W, w1.shape[0]))
    for tap in range(9):
        acc = fma(xp[:, tap // 3:tap // 3 + H, tap % 3:tap % 3 + W, None], w1[:, tap], acc)
    h = np.maximum(_f32(acc + b1), 0.0)
    w, b = folded(P, p + ".conv.3.weight", p + ".conv.4")
    h = np.maximum(_f32(_conv(_bf16(h), w, 1, order) + b), 0.0)
    sc = fma(x[..., None], P[p + ".shortcut.weight"].astype(np.float64).reshape(-1), P[p + ".shortcut.bias"])
    return _f32(h + sc)


def _pool(x, order):
    B, H, W, C = x.shape
    x = x.reshape(B, H // 2, 2, W // 2, 2, C)
    if order is None:
        return x.mean(axis=(2, 4))
    x = x.astype(np.float32)
    return (((x[:, :, 0, :, 0] + x[:, :, 0, :, 1]) + (x[:, :, 1, :, 0] + x[:, :, 1, :, 1])) * np.float32(0.25)).astype(np.float64)


def _gru_direction(P, suffix, x, reverse, order=None):
    """rmvpe_ref._gru_direction with the recurrent product on bf16 operands"""
    Wi, Wh, bi, bh = (P[f"fc.0.gru.{k}_l0{suffix}"].astype(np.float64)
                      for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
    H = Wh.shape[1]
    B, T, _ = x.shape
    xp = x @ Wi.T + bi
    WhT = np.ascontiguousarray(_bf16(Wh).T)
    h = np.zeros((B, H))
    out = np.zeros((B, T, H))
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        hp = _matmul(_bf16(h), WhT, H, order) + bh
        r = R._sigmoid(xp[:, t, :H] + hp[:, :H])
        z = R._sigmoid(xp[:, t, H:2 * H] + hp[:, H:2 * H])
        n = np.tanh(xp[:, t, 2 * H:] + r * hp[:, 2 * H:])
        h = _f32((1.0 - z) * n + z * h)
        out[:, t] = h
    return out


def e2e0(P, model, mel, conv=True, gru=True, order=None):
    """mel [B, n_mels, T] -> (feat [B, T, 3 n_mels], hidden [B, T, n_class]) of the bf16 modes in float64.
    ``conv`` / ``gru``: which of the two options is bf16 (both False is rmvpe_ref.e2e0); ``order``: see above."""
    L, nb = model["en_de_layers"], model["n_blocks"]
    block = (lambda p, x: _block(P, p, x, order)) if conv else (lambda p, x: R._block(P, p, x))
    raw = np.asarray(mel, np.float64).transpose(0, 2, 1)[..., None]
    x = R._bn(P, "unet.encoder.bn", raw)
    skips = []
    for i in range(L):
        for j in range(nb):
            if i == j == 0 and conv and order is not None:
                x = _first_block_f32(P, "unet.encoder.layers.0.conv.0", raw, order)
            else:
                x = block(f"unet.encoder.layers.{i}.conv.{j}", x)
        skips.append(x)
        x = _pool(x, order if conv else None)
    for i in range(model["inter_layers"]):
        for j in range(nb):
            x = block(f"unet.intermediate.layers.{i}.conv.{j}", x)
    for i in range(L):
        p = f"unet.decoder.layers.{i}"
        if conv:
            w, b = folded(P, p + ".conv1.0.weight", p + ".conv1.1", transposed=True)
            x = _f32(np.maximum(_conv_transpose(_bf16(_f32(x)), w, order) + b, 0.0))
        else:
            x = np.maximum(R._bn(P, p + ".conv1.1", R._conv_transpose(x, P[p + ".conv1.0.weight"])), 0.0)
        x = np.concatenate([x, skips[L - 1 - i]], axis=-1)
        for j in range(nb):
            x = block(f"{p}.conv2.{j}", x)
    x = R._conv(x, P["cnn.weight"], 1) + P["cnn.bias"].astype(np.float64)
    B, T, F, _ = x.shape
    feat = x.transpose(0, 1, 3, 2).reshape(B, T, 3 * F)
    if conv:
        feat = _f32(feat)
    if model["n_gru"]:
        if gru:
            g = np.concatenate([_gru_direction(P, "", feat, False, order),
                                _gru_direction(P, "_reverse", feat, True, order)], axis=-1)
        else:
            g = np.concatenate([R._gru_direction(P, "", feat, False), R._gru_direction(P, "_reverse", feat, True)], axis=-1)
        logits = g @ P["fc.1.weight"].astype(np.float64).T + P["fc.1.bias"].astype(np.float64)
    else:
        logits = feat @ P["fc.0.weight"].astype(np.float64).T + P["fc.0.bias"].astype(np.float64)
    return feat, R._sigmoid(logits)


# ---------------------------------------------------------------- shared by the CPU and the GPU tests
SMALL = ("rmvpe_shallow", "rmvpe_nogru", "rmvpe_slim")
ORDER_DRAWS = {True: 4, False: 2}      # f32 summation orders drawn per case: small nets, full-size nets
ORDER_FACTOR = 1.5


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@functools.lru_cache(maxsize=None)
def emulated(name, conv=True, gru=True):
    """(feat, hidden) of the emulation on the case's input, computed once per session and not to be written to."""
    out = e2e0(RC.case_params(name), RC.CASES[name][0], RC.case_mel(name), conv, gru)
    for x in out:
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def order_noise(name):
    """What the f32 summation order alone is worth on this case: {"feat", "hidden"} -> the largest rel-L2 distance,
    over ORDER_DRAWS seeded channel permutations, between the emulation summed in f32 and the one summed in double."""
    exact = dict(zip(("feat", "hidden"), emulated(name)))
    P, model, mel = RC.case_params(name), RC.CASES[name][0], RC.case_mel(name)
    worst = {"feat": 0.0, "hidden": 0.0}
    for seed in range(ORDER_DRAWS[name in SMALL]):
        got = dict(zip(("feat", "hidden"), e2e0(P, model, mel, order=np.random.default_rng(seed))))
        for k in worst:
            worst[k] = max(worst[k], rel_l2(got[k], exact[k]))
    return worst
