#!/usr/bin/env python
"""Time the native harmonic-noise separation (prodiff_amd.CascadedNet, pd_vr_separate) with HIP events: 1 and 8
utterances x 10 s at 44.1 kHz (862 frames, padded to 864 as predict_from_audio does), CascadedNet(2048, 512, 32, 128)
mono with synthetic weights.  Warm-up, then the median over --calls single calls; the same call replayed from one
captured single-stream graph (checked bit-equal); a per-kernel table from pd_profile_*; and the same computation
written with torch ops (torch.stft, F.conv2d, F.batch_norm, F.interpolate, nn.LSTM, torch.istft) in eager mode on
the same GPU.  Prints one JSON line per batch size.

    python tools/bench_vr.py [--calls 20] [--warmup 3] [--batches 1,8] [--seconds 10] [--no-torch]
    python tools/bench_vr.py --ragged N [--calls 20]
    python tools/bench_vr.py --dtype bf16 [...]
    python tools/bench_vr.py --check clip.wav [--ckpt model.pt]

--dtype bf16 (default fp32: the lines above as they always were) prints every line twice, first with the model in
fp32, then with ``set_compute_dtype("bf16")`` (a "dtype" key tells them apart; the bf16 line adds its harmonic part's
distance from the fp32 one and skips the torch comparison), --ragged N included.

--check WAV runs one clip (16- or 32-bit PCM or float WAV, mixed down to mono, taken as 44.1 kHz) in both modes, with
the checkpoint's model (``load_sep_model``; config.yaml beside it) or, without --ckpt, the synthetic-weight model,
and prints rel-L2 and max-rel of the harmonic part and of the aperiodic part, each against its own fp32 norm and peak,
and the largest difference of the get_breath and get_voicing curves (hop 512, window 2048, unnormalised dB).  With a
trained model the aperiodic part is far quieter than the harmonic one, so the same absolute error is a larger share
of it: this is the figure to judge the mode by, and the synthetic weights (|aperiodic| about |harmonic|) cannot show it.

--ragged N times ``CascadedNet.separate`` on clips of the first N lengths of tests/golden/ds_lengths.json (frames
times the hop, in samples) three ways: (a) one ragged call on the padded batch with ``lens``, (b) one call per clip
(the only way without ragged batches), (c) one equal-length call on the clips padded to the longest (its results
are not those of the clips alone).  (a) is checked bit-equal to (b) first.

The conv floor: 2 x output pixels x taps C_in C_out FLOP per conv on the f32 MFMA (157.3 TFLOP/s dense); the bf16
lines give the share of the bf16 MFMA's 2.5 PFLOP/s beside it.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import prodiff_amd  # noqa: E402
from prodiff_amd import _lib, synth  # noqa: E402
from prodiff_amd.vr import padded_frames  # noqa: E402

F32_MFMA_PEAK = 157.3e12
BF16_MFMA_PEAK = 2.5e15
FULL = dict(n_fft=2048, hop_length=512, nout=32, nout_lstm=128, is_mono=True)


def time_calls(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms = np.sort(np.array(ms))
    return float(np.median(ms)), float(ms[0]), float(ms[int(0.9 * (len(ms) - 1))])


def conv_flop(shapes, B, T, F_bins):
    """FLOP of every Conv2d the forward runs (aux_out is not run) for a [B, T, F_bins] spectrum."""
    level = {"enc1": 0, "enc2": 1, "enc3": 2, "enc4": 3, "enc5": 4, "aspp": 4, "dec4": 3, "dec3": 2, "dec2": 1,
             "lstm_dec2": 1, "dec1": 0}
    total = 0
    for k, s in shapes.items():
        if len(s) != 4 or k.startswith("aux_out"):
            continue
        part = k.split(".")
        bins = F_bins if part[0] in ("stg3_full_band_net", "out") else F_bins // 2
        name = part[2] if part[1] == "0" else part[1]
        lvl = level.get(name, 0)                      # the band tails and `out` run at full resolution
        pix = B * (T >> lvl) * (bins >> lvl)
        if name == "aspp" and ".conv1.1." in k:       # on the mean over the bins
            pix = B * (T >> lvl)
        total += 2 * pix * s[0] * s[1] * s[2] * s[3]
    return total


# ---------------------------------------------------------------- the same computation with torch ops
def torch_separate(P, lstms, a, wav):
    def cba(p, x, stride=1, pad=0, dil=1, leaky=False):
        y = F.conv2d(x, P[p + ".conv.0.weight"], None, stride, pad, dil)
        y = F.batch_norm(y, P[p + ".conv.1.running_mean"], P[p + ".conv.1.running_var"], P[p + ".conv.1.weight"],
                         P[p + ".conv.1.bias"], False, 0.0, 1e-5)
        return F.leaky_relu(y, 0.01) if leaky else F.relu(y)

    def dec(p, x, skip):
        x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
        return cba(p + ".conv1", torch.cat([x, skip], dim=1), 1, 1)

    def base(p, x):
        e = [cba(p + ".enc1", x, 1, 1)]
        for i in (2, 3, 4, 5):
            e.append(cba(f"{p}.enc{i}.conv2", cba(f"{p}.enc{i}.conv1", e[-1], 2, 1, leaky=True), 1, 1, leaky=True))
        e5 = e[4]
        feats = [cba(p + ".aspp.conv1.1", e5.mean(-2, keepdim=True)).repeat(1, 1, e5.shape[2], 1), cba(p + ".aspp.conv2", e5)]
        for i, d in zip((3, 4, 5), ((4, 2), (8, 4), (12, 6))):
            feats.append(cba(f"{p}.aspp.conv{i}", e5, 1, d, d))
        h = cba(p + ".aspp.bottleneck", torch.cat(feats, dim=1))
        h = dec(p + ".dec2", dec(p + ".dec3", dec(p + ".dec4", h, e[3]), e[2]), e[1])
        q = p + ".lstm_dec2"
        N, _, nbins, nframes = h.shape
        z = lstms[q](cba(q + ".conv", h)[:, 0].permute(2, 0, 1))[0]
        z = F.linear(z.reshape(-1, z.shape[-1]), P[q + ".dense.0.weight"], P[q + ".dense.0.bias"])
        z = F.relu(F.batch_norm(z, P[q + ".dense.1.running_mean"], P[q + ".dense.1.running_var"], P[q + ".dense.1.weight"],
                                P[q + ".dense.1.bias"], False, 0.0, 1e-5))
        h = torch.cat([h, z.reshape(nframes, N, 1, nbins).permute(1, 2, 3, 0)], dim=1)
        return dec(p + ".dec1", h, e[0])

    B, C, L = wav.shape
    n_fft, hop = a["n_fft"], a["hop_length"]
    T, Tl_pad, T_pad = padded_frames(L, hop)
    win = torch.hann_window(n_fft, device=wav.device)
    spec = torch.stft(F.pad(wav.reshape(B * C, L), (Tl_pad, T_pad - Tl_pad)), n_fft, hop, window=win, return_complex=True,
                      pad_mode="constant").reshape(B, C, n_fft // 2 + 1, T)
    x = torch.cat([spec.real, spec.imag], dim=1)[:, :, :n_fft // 2]
    bw = x.shape[2] // 2
    lo, hi = x[:, :, :bw], x[:, :, bw:]
    l1 = cba("stg1_low_band_net.1", base("stg1_low_band_net.0", lo))
    h1 = base("stg1_high_band_net", hi)
    aux1 = torch.cat([l1, h1], dim=2)
    l2 = cba("stg2_low_band_net.1", base("stg2_low_band_net.0", torch.cat([lo, l1], dim=1)))
    h2 = base("stg2_high_band_net", torch.cat([hi, h1], dim=1))
    f3 = base("stg3_full_band_net", torch.cat([x, aux1, torch.cat([l2, h2], dim=2)], dim=1))
    m = F.conv2d(f3, P["out.weight"])
    m = torch.complex(m[:, :C], m[:, C:])
    mag = m.abs()
    m = torch.tanh(mag) * m / (mag + 1e-8)
    m = torch.cat([m, m[:, :, -1:]], dim=2)
    y = torch.istft((spec * m).reshape(B * C, n_fft // 2 + 1, T), n_fft, hop, window=win)
    return y[:, Tl_pad:Tl_pad + L].reshape(B, C, L)


def dtypes_of(a):
    return ("fp32",) if a.dtype == "fp32" else ("fp32", "bf16")


def rel_errors(got, ref):
    """(rel-L2 against ref's norm, max|d| against ref's peak)"""
    d = (got.double() - ref.double())
    return float(d.norm() / ref.double().norm()), float(d.abs().max() / ref.abs().max())


def read_wav(path):
    """A PCM or float WAV as float32 mono in [-1, 1] and its sample rate (soundfile where installed, else the
    standard library's reader: 16- and 32-bit PCM)."""
    try:
        import soundfile
        x, sr = soundfile.read(path, dtype="float32", always_2d=True)
        return x.mean(axis=1), sr
    except ImportError:
        import wave
        with wave.open(path, "rb") as w:
            sr, ch, width, n = w.getframerate(), w.getnchannels(), w.getsampwidth(), w.getnframes()
            raw = w.readframes(n)
        if width not in (2, 4):
            raise SystemExit(f"{path}: {8 * width}-bit PCM is not read without the soundfile package")
        x = np.frombuffer(raw, dtype="<i2" if width == 2 else "<i4").astype(np.float32) / float(1 << (8 * width - 1))
        return x.reshape(-1, ch).mean(axis=1), sr


def check_clip(a):
    from prodiff_amd import curves
    from prodiff_amd.vr import load_sep_model
    dev = torch.device("cuda:0")
    wav, sr = read_wav(a.check)
    if a.ckpt:
        net = load_sep_model(a.ckpt, dev)
    else:
        net = prodiff_amd.CascadedNet(**FULL)
        shapes = synth.vr_param_shapes(FULL["n_fft"], FULL["nout"], FULL["nout_lstm"], FULL["is_mono"])
        net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_vr_params(shapes, a.seed).items()})
        net.to(dev)
    x = torch.from_numpy(np.ascontiguousarray(wav)).to(dev)[None, None].repeat(1, net.channels, 1)
    hop, win = 512, 2048
    mel_len = curves.num_frames(x.shape[-1], hop)
    smooth = curves.SinusoidalSmoothingConv1d(round(0.12 * sr / hop))
    out = {}
    for dt in ("fp32", "bf16"):
        y, ap_ = net.set_compute_dtype(dt).separate(x)
        sp, ap_ = y.mean(dim=1)[0], x[0, 0] - y.mean(dim=1)[0]
        out[dt] = (sp, ap_, curves.get_voicing(sp, mel_len, hop, win, smooth, norm=False, device=dev),
                   curves.get_breath(ap_, mel_len, hop, win, smooth, norm=False, device=dev))
    (sp, ap_, vo, br), (sp_b, ap_b, vo_b, br_b) = out["fp32"], out["bf16"]
    line = {"bench": "vr_check", "wav": os.path.basename(a.check), "samples": int(x.shape[-1]), "sr": sr,
            "model": "checkpoint" if a.ckpt else "synthetic weights", "device": torch.cuda.get_device_name(0),
            "aperiodic_over_harmonic_norm": round(float(ap_.norm() / sp.norm()), 4)}
    for key, got, ref in (("harmonic", sp_b, sp), ("aperiodic", ap_b, ap_)):
        rel, mx = rel_errors(got, ref)
        line[key + "_rel_l2"], line[key + "_max_rel"] = float(f"{rel:.3e}"), float(f"{mx:.3e}")
    line["voicing_max_db_diff"] = round(float((vo_b - vo).abs().max()), 4)
    line["breath_max_db_diff"] = round(float((br_b - br).abs().max()), 4)
    print(json.dumps(line), flush=True)
    net.close()


def bench_ragged(a):
    dev = torch.device("cuda:0")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "tests", "golden", "ds_lengths.json")) as f:
        ds = json.load(f)
    sr, hop = int(ds["sr"]), int(ds["hop"])
    frames = [int(v) for v in ds["frames"][:a.ragged]]
    if len(frames) < a.ragged:
        raise SystemExit(f"ds_lengths.json holds {len(frames)} lengths")
    lens = [n * hop for n in frames]
    net = prodiff_amd.CascadedNet(**FULL)
    shapes = synth.vr_param_shapes(FULL["n_fft"], FULL["nout"], FULL["nout_lstm"], FULL["is_mono"])
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_vr_params(shapes, a.seed).items()})
    net.to(dev)
    g = torch.Generator().manual_seed(0)
    clips = [((torch.rand(n, generator=g) * 2 - 1) * 0.3).to(dev)[None, None] for n in lens]
    padded = torch.zeros(len(clips), 1, max(lens), device=dev)
    for b, c in enumerate(clips):
        padded[b, :, :c.shape[-1]] = c[0]

    def ragged():
        return net.separate(padded, lens)

    def one_by_one():
        return [net.separate(c) for c in clips]

    def padded_call():
        return net.separate(padded)

    for dt in dtypes_of(a):
        net.set_compute_dtype(dt)
        y, ap_ = ragged()
        same = all(torch.equal(y[b, :, :n], r[0][0]) and torch.equal(ap_[b, :, :n], r[1][0])
                   for b, (n, r) in enumerate(zip(lens, one_by_one())))
        line = {"bench": "vr_ragged", "N": len(lens), "seconds": [round(n / sr, 2) for n in lens],
                "frames": [padded_frames(n, FULL["hop_length"])[0] for n in lens], "calls": a.calls,
                "device": torch.cuda.get_device_name(0), "lib": _lib.lib().pd_build_config().decode(),
                "ragged_equals_single_calls": bool(same)}
        if a.dtype != "fp32":
            line["dtype"] = dt
        for key, fn in (("ragged", ragged), ("single_calls", one_by_one), ("padded", padded_call)):
            med, best, p90 = time_calls(fn, a.calls, a.warmup)
            line[key + "_ms"] = {"median": round(med, 3), "min": round(best, 3), "p90": round(p90, 3)}
        print(json.dumps(line), flush=True)
    net.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ragged", type=int, default=0, metavar="N")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--seed", type=int, default=54)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--dtype", choices=("fp32", "bf16"), default="fp32")
    ap.add_argument("--check", metavar="WAV")
    ap.add_argument("--ckpt", metavar="MODEL.PT")
    a = ap.parse_args()
    if a.check:
        return check_clip(a)
    if a.ragged:
        return bench_ragged(a)
    dev = torch.device("cuda:0")
    Lw = int(round(a.seconds * 44100))
    shapes = synth.vr_param_shapes(FULL["n_fft"], FULL["nout"], FULL["nout_lstm"], FULL["is_mono"])
    host = synth.synth_vr_params(shapes, a.seed)
    net = prodiff_amd.CascadedNet(**FULL)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in host.items()})
    net.to(dev)
    P = lstms = None
    if not a.no_torch:
        P = {k: torch.from_numpy(v).to(dev) for k, v in host.items()}
        lstms = {}
        for k in host:
            if k.endswith(".lstm.weight_ih_l0"):
                q = k[:-len(".lstm.weight_ih_l0")]
                m = torch.nn.LSTM(host[k].shape[1], host[k].shape[0] // 4, bidirectional=True).to(dev).eval()
                m.load_state_dict({n[len(q) + 6:]: v for n, v in P.items() if n.startswith(q + ".lstm.")})
                lstms[q] = m
    for B in [int(v) for v in a.batches.split(",")]:
        g = torch.Generator().manual_seed(B)
        t = torch.arange(Lw) / 44100.0
        wav = torch.stack([(0.2 * sum(torch.sin(2 * np.pi * (200.0 + 30 * b) * k * t) / k for k in range(1, 9))
                            + 0.02 * torch.randn(Lw, generator=g)) for b in range(B)])[:, None].to(dev)
        T = padded_frames(Lw, FULL["hop_length"])[0]
        y32 = None
        for dt in dtypes_of(a):
            net.set_compute_dtype(dt)
            y, ap_ = net.separate(wav)
            line = {"bench": "vr", "B": B, "samples": Lw, "T": T, "calls": a.calls, "device": torch.cuda.get_device_name(0),
                    "lib": _lib.lib().pd_build_config().decode()}
            if a.dtype != "fp32":
                line["dtype"] = dt
            if dt == "fp32":
                y32 = y
            else:
                rel, mx = rel_errors(y, y32)
                line.update(harmonic_rel_l2_vs_fp32=float(f"{rel:.3e}"), harmonic_max_rel_vs_fp32=float(f"{mx:.3e}"))
            med, best, p90 = time_calls(lambda: net.separate(wav), a.calls, a.warmup)
            line.update(native_ms_median=round(med, 3), native_ms_min=round(best, 3), native_ms_p90=round(p90, 3))
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out, out_ap = net.separate(wav)
            gm, gb, _ = time_calls(graph.replay, a.calls, a.warmup)
            line.update(graph_ms_median=round(gm, 3), graph_ms_min=round(gb, 3),
                        graph_equals_eager=bool(torch.equal(out, y) and torch.equal(out_ap, ap_)))
            del graph, out, out_ap
            n_prof = 3
            _lib.profile_enable(True)
            for _ in range(n_prof):
                net.separate(wav)
            torch.cuda.synchronize()
            prof = _lib.profile_summary()
            _lib.profile_enable(False)
            line["kernels_ms_per_call"] = {k: [c // n_prof, round(t_ / n_prof, 4)] for k, (c, t_) in sorted(prof.items())}
            conv_tags = ("vr_enc", "vr_dec", "vr_aspp", "vr_tail", "vr_out", "vr_lstm_conv")
            conv_ms = sum(t_ for k, (c, t_) in prof.items() if k.startswith(conv_tags) and k != "vr_aspp_mean") / n_prof
            flop = conv_flop(shapes, B, T, FULL["n_fft"] // 2)
            line.update(conv_gflop=round(flop / 1e9, 1), conv_ms=round(conv_ms, 3),
                        conv_f32_mfma_peak_fraction=round(flop / (conv_ms * 1e-3) / F32_MFMA_PEAK, 4),
                        conv_floor_ms_at_peak=round(flop / F32_MFMA_PEAK * 1e3, 3))
            if dt == "bf16":
                line["conv_bf16_mfma_peak_fraction"] = round(flop / (conv_ms * 1e-3) / BF16_MFMA_PEAK, 4)
            if not a.no_torch and dt == "fp32":
                try:
                    with torch.no_grad():
                        ref = torch_separate(P, lstms, FULL, wav)
                        line["torch_max_abs_diff"] = float((ref - y).abs().max())
                        tm, tb, _ = time_calls(lambda: torch_separate(P, lstms, FULL, wav), max(a.calls // 4, 5), 2)
                    line["torch_ms_median"], line["torch_ms_min"] = round(tm, 3), round(tb, 3)
                    del ref
                except Exception as e:
                    line["torch_error"] = f"{type(e).__name__}: {e}"[:300]
            print(json.dumps(line), flush=True)
        torch.cuda.empty_cache()
    net.close()


if __name__ == "__main__":
    main()
