"""Bit-for-bit comparison of every native handle kind across two library builds (GPU box).

A change meant to keep every value -- a reordered schedule, an interleave of independent MFMA chains, a rewrite
of the create-time packing -- is checked here against the library it replaces.  Each case builds one handle at the
small dims the GPU tests use, once per branch of its create walk, runs it once and records the output together with
``pd_live_device_bytes()`` right after the create: equal outputs and equal live bytes say that every weight kept
its place in the pool.

usage: python tools/bitcmp.py <out.npz> [case-name-prefix ...]   (PRODIFF_HIP_LIB selects the library)
       python tools/bitcmp.py --compare <a.npz> <b.npz>

Build the other library with tools/build_rev_lib.sh <rev>.  The FastDiff sampler cases (dense, ragged and the C3
shape, lvc_ps 0 and 1) are the ones this tool started with.
"""
import gc
import sys

import numpy as np

FD_SAMPLES = [("dense_2x67", 2, 67, None), ("ragged_3x90", 3, 90, [90, 41, 7]), ("c3_8x861", 8, 861, None)]


def cases():
    """name -> function(rec): builds the case's module, calls rec.created() once its handle exists and returns
    {output name: tensor or array}."""
    import torch
    from prodiff_amd import FastDiff, WaveNet, synth
    dev = torch.device("cuda:0")

    def tt(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def load(m, params):
        m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
        return m.to(dev)

    out = {}

    # ---- WaveNet, C = H = 256: bf16 builds the fragment-order buffers
    def wavenet(dtype):
        def run(rec):
            m = load(WaveNet(80, 256, 2, 256, 1), synth.synth_params(synth.wavenet_param_shapes(80, 256, 2, 256), 3))
            m.set_compute_dtype(dtype).handle()
            rec.created()
            return {"out": m(tt(synth.synth_inputs(1, (1, 1, 80, 64))), tt(np.array([2.0], np.float32)),
                             tt(synth.synth_inputs(2, (1, 256, 64))))}
        return run
    for dt in ("fp32", "bf16"):
        out[f"wavenet_{dt}"] = wavenet(dt)

    # ---- FastDiff: the eps network with 3 blocks and with 1, then the bf16 sampler
    def fastdiff(ratios, dtype):
        def run(rec):
            m = load(FastDiff(upsample_ratios=ratios),
                     synth.synth_params(synth.fastdiff_param_shapes(upsample_ratios=ratios), 31))
            m.set_compute_dtype(dtype).handle()
            rec.created()
            Tc, hop = 16, int(np.prod(ratios))
            return {"eps": m((tt(synth.synth_inputs(3, (1, 1, Tc * hop))),
                              tt(synth.synth_inputs(4, (1, 80, Tc), loc=-5.0, scale=2.0)),
                              tt(np.array([[23.4676]], np.float32))))}
        return run
    for nb, ratios in ((3, (8, 8, 4)), (1, (8,))):
        for dt in ("fp32", "bf16"):
            out[f"fastdiff_nb{nb}_{dt}"] = fastdiff(ratios, dt)

    def fd_sample(B, Tc, lens):
        def run(rec):
            from prodiff_amd.schedules import fastdiff_infer_params, fastdiff_reverse_schedule, fastdiff_train_alpha
            b, a, s, st = fastdiff_infer_params(fastdiff_reverse_schedule(4), fastdiff_train_alpha())
            m = load(FastDiff(), synth.synth_params(synth.fastdiff_param_shapes(), 31)).set_compute_dtype("bf16")
            m.handle()
            rec.created()
            mel = tt(synth.synth_inputs(80 + B, (B, Tc, 80), loc=-5.0, scale=2.0))
            res = {}
            for ps in (0, 1):
                m.set_options(lvc_ps=ps)
                res[f"ps{ps}"] = m.sample(mel, b, a, s, st, lens=lens, seed=77)
            return res
        return run
    for name, B, Tc, lens in FD_SAMPLES:
        out[f"fdsample_{name}"] = fd_sample(B, Tc, lens)

    # ---- NSF-HiFiGAN, ResBlock1 and ResBlock2
    def nsf(case, dtype):
        def run(rec):
            from prodiff_amd.nsf_hifigan import Generator
            from tests.nsf_cases import load as nsf_load
            h, io, seed = nsf_load(case)
            m = load(Generator(h), synth.synth_params(synth.nsf_param_shapes(**h), seed)).eval()
            m.set_compute_dtype(dtype).handle()
            rec.created()
            return {"wav": m.synthesize(tt(io["mel"]), tt(io["f0"]), 2.30259, rand_ini=tt(io["rand_ini"]),
                                        noise=tt(io["noise"]))}
        return run
    for rb, case in ((1, "nsf_c64_r8822"), (2, "nsf_c32_r44_rb2")):
        for dt in ("fp32", "bf16"):
            out[f"nsf_rb{rb}_{dt}"] = nsf(case, dt)

    # ---- the condition encoder: every optional parameter on, each off, and the gender ids
    def cond(dtype, **flags):
        def run(rec):
            from tests.test_gpu_cond import teacher_for
            hp = dict(synth.COND_DEFAULTS, enc_layers=2, num_spk=2, num_langs=3, **flags)
            V = 20
            t = teacher_for(hp, synth.synth_cond_params(synth.cond_param_shapes(V, **hp), 3), V)
            t.set_compute_dtype(dtype).cond_handle()
            rec.created()
            x = synth.synth_cond_inputs(8, [7, 4], V, 2, 3)
            for flag, key in (("use_spk_id", "spk_embed_id"), ("use_voicing_embed", "voicing"),
                              ("use_breath_embed", "breath")):
                if not hp[flag]:
                    x.pop(key)
            if hp["use_gender_id"]:
                x["gender_embed_id"] = np.array([1, 2], np.int64)
            x = {k: tt(v) for k, v in x.items()}
            c, e = t.forward_condition(x.pop("txt_tokens"), x.pop("mel2ph"), x.pop("f0"), return_encoder=True, **x)
            return {"cond": c, "enc": e}
        return run
    out["cond_all_fp32"] = cond("fp32")
    out["cond_all_bf16"] = cond("bf16")
    for flag in ("use_dur_embed", "use_spk_id", "use_voicing_embed", "use_breath_embed"):
        out[f"cond_no_{flag[4:]}"] = cond("fp32", **{flag: False})
    out["cond_gender"] = cond("fp32", use_gender_id=True)

    # ---- the variance predictors' encoders
    def pitch(name, dtype):
        def run(rec):
            from tests import variance_cases as VC
            from tests.test_gpu_variance import pitch_model
            m = pitch_model(name).set_compute_dtype(dtype)
            m.cond_handle()
            rec.created()
            return {"cond": m.forward_condition(**{k: tt(v) for k, v in VC.pitch_case(name)[2].items()})}
        return run

    def dur(dtype):
        def run(rec):
            from tests import variance_cases as VC
            from tests.test_gpu_variance import dur_model
            m = dur_model("dur_small").set_compute_dtype(dtype)
            m.dur_handle()
            rec.created()
            d, log = m(**{k: tt(v) for k, v in VC.dur_case("dur_small")[2].items()}, return_log=True)
            return {"dur": d, "log": log}
        return run
    for dt in ("fp32", "bf16"):
        out[f"pitch_spk_{dt}"] = pitch("pitchcond_small", dt)
        out[f"dur_{dt}"] = dur(dt)
    out["pitch_nospk_fp32"] = pitch("pitchcond_nospk", "fp32")

    # ---- RMVPE with and without the GRU, the separation net
    def rmvpe(name):
        def run(rec):
            import prodiff_amd
            from tests import rmvpe_cases as RC
            a = RC.CASES[name][0]
            net = load(prodiff_amd.E2E0(a["n_blocks"], a["n_gru"], (2, 2), a["en_de_layers"], a["inter_layers"], 1,
                                        a["en_out_channels"]), RC.case_params(name))
            net.handle()
            rec.created()
            hidden, feat = net.forward_features(tt(RC.case_mel(name)))
            return {"hidden": hidden, "feat": feat}
        return run
    out["rmvpe_gru"] = rmvpe("rmvpe_shallow")
    out["rmvpe_nogru"] = rmvpe("rmvpe_nogru")

    def vr(rec):
        import prodiff_amd
        from tests import vr_cases as VC
        net = load(prodiff_amd.CascadedNet(**VC.model_args("vr_tiny_mono")), VC.case_params("vr_tiny_mono"))
        net.handle()
        rec.created()
        return {"y": net.predict_from_audio(tt(VC.case_wav("vr_tiny_mono")))}
    out["vr_tiny_mono"] = vr

    # ---- the table-only handles: their creates run inside the first call
    def mel(rec):
        from prodiff_amd import STFT
        s = STFT(44100, 128, 2048, 2048, 512, 40, 16000)
        m = s.get_mel(tt(synth.synth_inputs(11, (2, 8192), scale=0.1)))
        rec.created()
        return {"mel": m}
    out["mel"] = mel

    def resample(rec):
        from prodiff_amd import KAISER_BEST, Resample
        r = Resample(48000, 44100, **KAISER_BEST)
        y = r(tt(synth.synth_inputs(12, (2, 4000), scale=0.1)))
        rec.created()
        return {"y": y}
    out["resample"] = resample

    def curves(rec):
        import prodiff_amd
        from prodiff_amd import curves as CV
        CV.close_all()
        hop, win, sr, L = 512, 2048, 44100, 512 * 24
        f0 = np.full((2, L // hop + 1), 220.0, np.float32)
        y = prodiff_amd.get_kth_harmonic(0, tt(synth.synth_inputs(13, (2, L), scale=0.1)), tt(f0), hop, win, sr)
        rec.created()
        return {"y": y}
    out["curves"] = curves
    return out


class Rec:
    def __init__(self, lib):
        self.lib, self.base, self.live = lib, lib.pd_live_device_bytes(), None

    def created(self):
        self.live = self.lib.pd_live_device_bytes() - self.base


def run(out, only):
    import torch
    sys.path.insert(0, ".")
    from prodiff_amd import _lib
    res = {}
    for name, fn in cases().items():
        if only and not any(name.startswith(p) for p in only):
            continue
        gc.collect()
        rec = Rec(_lib.lib())
        outs = fn(rec)
        torch.cuda.synchronize()
        res[f"{name}/live_bytes"] = np.array(rec.live, np.int64)
        for k, v in outs.items():
            res[f"{name}/{k}"] = v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)
        peak = max(float(np.abs(res[f"{name}/{k}"]).max()) for k in outs)
        print(f"{name}: live {rec.live} B, {sorted(outs)}, max |x| {peak:.4g}", flush=True)
        del outs
        np.savez(out, **res)   # after every case: a run that ends early leaves what it had


def compare(fa, fb):
    A, Bz = np.load(fa), np.load(fb)
    bad = 0
    for k in sorted(set(A.files) | set(Bz.files)):
        if k not in A.files or k not in Bz.files:
            print(f"{k}: MISSING from {fb if k in A.files else fa}")
            bad += 1
        elif k.endswith("/live_bytes"):
            same = int(A[k]) == int(Bz[k])
            print(f"{k}: {'equal' if same else 'DIFFERENT'} ({int(A[k])} / {int(Bz[k])})")
            bad += not same
        else:
            same = A[k].shape == Bz[k].shape and A[k].tobytes() == Bz[k].tobytes()
            d = np.abs(A[k].astype(np.float64) - Bz[k].astype(np.float64)).max() if A[k].shape == Bz[k].shape else np.inf
            print(f"{k}: {'bit-identical' if same else 'DIFFERENT'} (max |d| {d:.3g})")
            bad += not same
    print(f"{len(A.files)} / {len(Bz.files)} arrays, {bad} differ")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        compare(sys.argv[2], sys.argv[3])
    else:
        run(sys.argv[1], sys.argv[2:])
