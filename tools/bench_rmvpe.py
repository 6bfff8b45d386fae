#!/usr/bin/env python
"""Time the native RMVPE network (prodiff_amd.E2E0, pd_rmvpe_forward) with HIP events: 8 utterances x 10 s at
16 kHz (1001 frames, zero-padded to 1024 as RMVPE.mel2hidden does), E2E0(4, 1, (2, 2)) with synthetic weights.
Warm-up, then the median over --calls single calls; the same call replayed from one captured graph; a per-kernel
table from pd_profile_*; the front end (centred mel) and the decode beside it; and the same network written
with torch ops (F.conv2d, F.batch_norm, F.conv_transpose2d, nn.GRU) in eager mode on the same GPU.  Prints one
JSON line.

    python tools/bench_rmvpe.py [--calls 100] [--warmup 5] [--batch 8] [--seconds 10] [--no-torch] [--dtype bf16]
    python tools/bench_rmvpe.py --ragged N [--calls 30] [--dtype bf16]
    python tools/bench_rmvpe.py --check clip.wav [--ckpt model.pt]

--dtype bf16 adds, beside the fp32 figures, the same call in the bf16 mode (``E2E0.set_compute_dtype("bf16")``: "bf16"
in the JSON line, with its own per-kernel table) and with each of the two options switched alone ("bf16_convs_only",
"bf16_recurrence_only"); with --ragged it adds the ragged call's bf16 line.

--check runs one clip (any sample rate, mono or the first channel) through the extractor in fp32 and in the three bf16
modes and prints, per mode against fp32: rel-L2 of ``hidden``, the frames whose argmax or voicing flag differ, the f0
difference in cents (max and median over the commonly voiced frames) and the smallest top-two salience margin of the
fp32 run.  Without --ckpt the weights are synthetic, whose margins are far smaller than a trained model's.

--ragged N times ``RMVPE.get_pitch_batch`` (44.1 kHz audio to f0 on the mel grid, hop 512) on clips of the first N
lengths of tests/golden/ds_lengths.json three ways: (a) one ragged call on the list of clips, (b) one call per clip
(the only way without ragged batches), (c) one equal-length call on the clips padded to the longest (its results
are not the clips' own; only its time is of interest).  Prints one JSON line with median, min and p90 of each.

The conv floor: 2 x pixels x 9 C_in C_out FLOP per conv on the f32 MFMA (157.3 TFLOP/s dense).
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
from prodiff_amd import rmvpe as RM  # noqa: E402

F32_MFMA_PEAK = 157.3e12
FULL = dict(synth.RMVPE_DEFAULTS)


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


def conv_flop(shapes, model, B, T, n_mels=128):
    """FLOP of every conv (3x3, 1x1 shortcut, transposed) for a [B, T, n_mels] input."""
    L = model["en_de_layers"]
    total = 0
    for k, s in shapes.items():
        if len(s) != 4:
            continue
        part = k.split(".")
        if part[1] == "encoder":
            lvl = int(part[3])
        elif part[1] == "intermediate":
            lvl = L
        elif part[1] == "decoder":
            lvl = L - 1 - int(part[3])
        else:
            lvl = 0                                   # cnn
        pix = B * (T >> lvl) * (n_mels >> lvl)
        if ".conv1.0." in k:                          # transposed: each output pixel sees 9/4 taps on average
            total += 2 * pix * s[0] * s[1] * 9 // 4
        else:
            total += 2 * pix * s[0] * s[1] * s[2] * s[3]
    return total


# ---------------------------------------------------------------- the same network with torch ops
def torch_e2e0(P, model, mel, gru):
    def bn(p, x):
        return F.batch_norm(x, P[p + ".running_mean"], P[p + ".running_var"], P[p + ".weight"], P[p + ".bias"], False, 0.0, 1e-5)

    def block(p, x):
        h = F.relu(bn(p + ".conv.1", F.conv2d(x, P[p + ".conv.0.weight"], padding=1)))
        h = F.relu(bn(p + ".conv.4", F.conv2d(h, P[p + ".conv.3.weight"], padding=1)))
        if p + ".shortcut.weight" in P:
            return h + F.conv2d(x, P[p + ".shortcut.weight"], P[p + ".shortcut.bias"])
        return h + x

    L, nb = model["en_de_layers"], model["n_blocks"]
    x = bn("unet.encoder.bn", mel.transpose(-1, -2).unsqueeze(1))
    skips = []
    for i in range(L):
        for j in range(nb):
            x = block(f"unet.encoder.layers.{i}.conv.{j}", x)
        skips.append(x)
        x = F.avg_pool2d(x, 2)
    for i in range(model["inter_layers"]):
        for j in range(nb):
            x = block(f"unet.intermediate.layers.{i}.conv.{j}", x)
    for i in range(L):
        p = f"unet.decoder.layers.{i}"
        x = F.relu(bn(p + ".conv1.1", F.conv_transpose2d(x, P[p + ".conv1.0.weight"], stride=2, padding=1, output_padding=1)))
        x = torch.cat((x, skips[-1 - i]), dim=1)
        for j in range(nb):
            x = block(f"{p}.conv2.{j}", x)
    x = F.conv2d(x, P["cnn.weight"], P["cnn.bias"], padding=1).transpose(1, 2).flatten(-2)
    return torch.sigmoid(F.linear(gru(x)[0], P["fc.1.weight"], P["fc.1.bias"]))


def measure_network(net, mel, a, T):
    """median / min / p90 of one forward call, the per-kernel table and what follows from it"""
    out = {}
    med, best, p90 = time_calls(lambda: net.forward_time_major(mel), a.calls, a.warmup)
    out.update(native_ms_median=round(med, 3), native_ms_min=round(best, 3), native_ms_p90=round(p90, 3))
    n_prof = 5
    _lib.profile_enable(True)
    for _ in range(n_prof):
        net.forward_time_major(mel)
    torch.cuda.synchronize()
    prof = _lib.profile_summary()
    _lib.profile_enable(False)
    out["kernels_ms_per_call"] = {k: [c // n_prof, round(t / n_prof, 4)] for k, (c, t) in sorted(prof.items())}
    out["conv_ms"] = round(sum(t for k, (c, t) in prof.items() if k.startswith("rmvpe_conv")) / n_prof, 3)
    lvl = {}
    for k, (c, t) in prof.items():
        if k.startswith("rmvpe_conv") and k[-2] == "l" and k[-1].isdigit():
            lvl[k[-2:]] = lvl.get(k[-2:], 0.0) + t / n_prof
    out["conv_ms_per_level"] = {k: round(v, 3) for k, v in sorted(lvl.items())}
    if "rmvpe_gru" in prof:
        out["gru_us_per_step"] = round(prof["rmvpe_gru"][1] / n_prof / T * 1e3, 3)
    return out


def load_wav(path):
    """-> (float32 mono [n], sample rate) of a PCM or float .wav, without torchaudio"""
    import wave
    try:
        with wave.open(path, "rb") as w:
            sr, ch, width, n = w.getframerate(), w.getnchannels(), w.getsampwidth(), w.getnframes()
            raw = w.readframes(n)
        if width == 2:
            x = np.frombuffer(raw, "<i2").astype(np.float32) / 32768.0
        elif width == 4:
            x = np.frombuffer(raw, "<i4").astype(np.float32) / 2147483648.0
        elif width == 3:
            b = np.frombuffer(raw, np.uint8).reshape(-1, 3).astype(np.int32)
            x = ((b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)) << 8 >> 8).astype(np.float32) / 8388608.0
        else:
            x = (np.frombuffer(raw, np.uint8).astype(np.float32) - 128.0) / 128.0
        return np.ascontiguousarray(x.reshape(-1, ch)[:, 0]), sr
    except wave.Error:
        from scipy.io import wavfile          # float .wav files
        sr, x = wavfile.read(path)
        x = x if x.ndim == 1 else x[:, 0]
        return np.ascontiguousarray(x, np.float32), int(sr)


def check_clip(a):
    dev = torch.device("cuda:0")
    audio, sr = load_wav(a.check)
    pe = RM.RMVPE({}, model_path=a.ckpt)
    if a.ckpt is None:
        pe.model.load_state_dict({k: torch.from_numpy(v) for k, v in
                                  synth.synth_rmvpe_params(synth.rmvpe_param_shapes(**FULL), a.seed).items()})
    pe.model.to(dev)
    wav = torch.from_numpy(audio)[None].to(dev)
    thred = 0.03

    def run(conv, gru):
        hidden = pe.set_compute_dtype(conv, gru)._hidden_from_audio(wav, sr)[0].clone()
        return hidden.double().cpu().numpy(), RM.to_local_average_f0(hidden[None], thred=thred)[0].double().cpu().numpy()

    h32, f32_ = run("fp32", "fp32")
    top = np.sort(h32, axis=-1)
    line = {"bench": "rmvpe_check", "clip": os.path.basename(a.check), "sr": sr, "frames": int(h32.shape[0]),
            "weights": "checkpoint" if a.ckpt else "synthetic", "voiced_fp32": int((f32_ > 0).sum()),
            "top_two_margin_fp32": {"min": float((top[:, -1] - top[:, -2]).min()),
                                    "median": float(np.median(top[:, -1] - top[:, -2]))}}
    for key, conv, gru in (("bf16", "bf16", "bf16"), ("bf16_convs_only", "bf16", "fp32"),
                           ("bf16_recurrence_only", "fp32", "bf16")):
        h, f = run(conv, gru)
        both = (f > 0) & (f32_ > 0)
        c = 1200.0 * np.abs(np.log2(f[both] / f32_[both])) if both.any() else np.zeros(1)
        line[key] = {"hidden_rel_l2": float(np.linalg.norm(h - h32) / np.linalg.norm(h32)),
                     "argmax_differs": int((h.argmax(-1) != h32.argmax(-1)).sum()),
                     "voicing_differs": int(((f > 0) != (f32_ > 0)).sum()),
                     "f0_cents_max": float(c.max()), "f0_cents_median": float(np.median(c))}
        print(f"{key:>22}: hidden rel-L2 {line[key]['hidden_rel_l2']:.3e}, argmax differs on "
              f"{line[key]['argmax_differs']} and voicing on {line[key]['voicing_differs']} of {h.shape[0]} frames, f0 "
              f"{line[key]['f0_cents_max']:.4f} cents max / {line[key]['f0_cents_median']:.4f} median over "
              f"{int(both.sum())} voiced frames", flush=True)
    print(json.dumps(line), flush=True)
    pe.model.close()
    pe.mel_extractor.close()


def bench_ragged(a):
    dev = torch.device("cuda:0")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "tests", "golden", "ds_lengths.json")) as f:
        ds = json.load(f)
    sr, hop = int(ds["sr"]), int(ds["hop"])
    lengths = [int(v) for v in ds["frames"][:a.ragged]]
    if len(lengths) < a.ragged:
        raise SystemExit(f"ds_lengths.json holds {len(lengths)} lengths")
    pe = RM.RMVPE({})
    pe.model.load_state_dict({k: torch.from_numpy(v) for k, v in
                              synth.synth_rmvpe_params(synth.rmvpe_param_shapes(**FULL), a.seed).items()})
    pe.model.to(dev)
    g = torch.Generator().manual_seed(0)
    clips = [((torch.rand(n * hop, generator=g) * 2 - 1) * 0.3).to(dev) for n in lengths]
    padded = torch.zeros(len(clips), max(lengths) * hop, device=dev)
    for b, c in enumerate(clips):
        padded[b, :c.numel()] = c
    singles = [c[None] for c in clips]

    def ragged():
        return pe.get_pitch_batch(clips, sr, lengths, hop_size=hop)

    def one_by_one():
        return [pe.get_pitch_batch(c, sr, n, hop_size=hop) for c, n in zip(singles, lengths)]

    def padded_call():
        return pe.get_pitch_batch(padded, sr, max(lengths), hop_size=hop)

    f0, uv = ragged()
    same = all(torch.equal(f0[b, :n], r[0][0]) and torch.equal(uv[b, :n], r[1][0])
               for b, (n, r) in enumerate(zip(lengths, one_by_one())))
    line = {"bench": "rmvpe_ragged", "N": len(lengths), "seconds": [round(n * hop / sr, 2) for n in lengths],
            "calls": a.calls, "device": torch.cuda.get_device_name(0), "lib": _lib.lib().pd_build_config().decode(),
            "ragged_equals_single_calls": bool(same)}
    for key, fn in (("ragged", ragged), ("single_calls", one_by_one), ("padded", padded_call)):
        med, best, p90 = time_calls(fn, a.calls, a.warmup)
        line[key + "_ms"] = {"median": round(med, 3), "min": round(best, 3), "p90": round(p90, 3)}
    if a.dtype == "bf16":
        for key, conv, gru in (("ragged_bf16", "bf16", "bf16"), ("ragged_bf16_convs_only", "bf16", "fp32"),
                               ("ragged_bf16_recurrence_only", "fp32", "bf16")):
            pe.set_compute_dtype(conv, gru)
            med, best, p90 = time_calls(ragged, a.calls, a.warmup)
            line[key + "_ms"] = {"median": round(med, 3), "min": round(best, 3), "p90": round(p90, 3)}
            if key == "ragged_bf16":
                _lib.profile_enable(True)
                for _ in range(5):
                    ragged()
                torch.cuda.synchronize()
                prof = _lib.profile_summary()
                _lib.profile_enable(False)
                line["ragged_bf16_kernels_ms_per_call"] = {k: [c // 5, round(t / 5, 4)] for k, (c, t) in sorted(prof.items())
                                                           if k.startswith("rmvpe")}
        pe.set_compute_dtype("fp32")
    print(json.dumps(line), flush=True)
    pe.model.close()
    pe.mel_extractor.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ragged", type=int, default=0, metavar="N")
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--seed", type=int, default=44)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--dtype", choices=("fp32", "bf16"), default="fp32")
    ap.add_argument("--check", metavar="CLIP.wav")
    ap.add_argument("--ckpt", metavar="MODEL.pt")
    a = ap.parse_args()
    if a.check:
        return check_clip(a)
    if a.ragged:
        return bench_ragged(a)
    dev = torch.device("cuda:0")
    B, Lw = a.batch, int(round(a.seconds * 16000))
    shapes = synth.rmvpe_param_shapes(**FULL)
    host = synth.synth_rmvpe_params(shapes, a.seed)
    net = prodiff_amd.E2E0(FULL["n_blocks"], FULL["n_gru"], (2, 2))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in host.items()})
    net.to(dev)
    g = torch.Generator().manual_seed(0)
    wav = ((torch.rand(B, Lw, generator=g) * 2 - 1) * 0.3).to(dev)
    ms_ = RM.MelSpectrogram(128, 16000, 1024, 160, None, 30, 8000)
    mel = ms_.forward_time_major(wav)
    frames = mel.shape[1]
    mel = F.pad(mel, (0, 0, 0, -frames % 32)).contiguous()
    T = mel.shape[1]
    hidden = net.forward_time_major(mel)
    line = {"bench": "rmvpe", "B": B, "samples": Lw, "frames": frames, "T": T, "calls": a.calls,
            "device": torch.cuda.get_device_name(0), "lib": _lib.lib().pd_build_config().decode()}
    line.update(measure_network(net, mel, a, T))
    conv_ms = line["conv_ms"]
    line["mel_ms_median"] = round(time_calls(lambda: ms_.forward_time_major(wav), a.calls, a.warmup)[0], 4)
    line["decode_ms_median"] = round(time_calls(lambda: RM.to_local_average_f0(hidden), a.calls, a.warmup)[0], 4)
    # the same call from one captured graph
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = net.forward_time_major(mel)
    gm, gb, _ = time_calls(graph.replay, a.calls, a.warmup)
    line.update(graph_ms_median=round(gm, 3), graph_ms_min=round(gb, 3), graph_equals_eager=bool(torch.equal(out, hidden)))
    flop = conv_flop(shapes, FULL, B, T)
    line.update(conv_gflop=round(flop / 1e9, 1),
                conv_f32_mfma_peak_fraction=round(flop / (conv_ms * 1e-3) / F32_MFMA_PEAK, 4),
                conv_floor_ms_at_peak=round(flop / F32_MFMA_PEAK * 1e3, 3))
    if a.dtype == "bf16":
        for key, conv, gru in (("bf16", "bf16", "bf16"), ("bf16_convs_only", "bf16", "fp32"),
                               ("bf16_recurrence_only", "fp32", "bf16")):
            hb = net.set_compute_dtype(conv, gru).forward_time_major(mel)
            line[key] = measure_network(net, mel, a, T)
            line[key]["hidden_rel_l2_to_fp32"] = float((hb - hidden).norm() / hidden.norm())
            if key != "bf16":
                del line[key]["kernels_ms_per_call"]
        net.set_compute_dtype("fp32")
        line["fp32_bit_equal_after_the_switches"] = bool(torch.equal(net.forward_time_major(mel), hidden))
    if not a.no_torch:
        try:
            P = {k: torch.from_numpy(v).to(dev) for k, v in host.items()}
            gru = torch.nn.GRU(384, 256, num_layers=1, batch_first=True, bidirectional=True).to(dev).eval()
            gru.load_state_dict({k[len("fc.0.gru."):]: v for k, v in P.items() if k.startswith("fc.0.gru.")})
            mel_ct = mel.transpose(1, 2).contiguous()
            with torch.no_grad():
                ref = torch_e2e0(P, FULL, mel_ct, gru)
                line["torch_max_abs_diff"] = float((ref - hidden).abs().max())
                tm, tb, _ = time_calls(lambda: torch_e2e0(P, FULL, mel_ct, gru), max(a.calls // 5, 10), 3)
            line["torch_ms_median"], line["torch_ms_min"] = round(tm, 3), round(tb, 3)
        except Exception as e:
            line["torch_error"] = f"{type(e).__name__}: {e}"[:300]
    print(json.dumps(line), flush=True)
    net.close()
    ms_.close()


if __name__ == "__main__":
    main()
