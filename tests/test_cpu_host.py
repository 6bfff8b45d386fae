"""CPU-only checks: the C-ABI library loads and exports what include/*.h declares,
the host-side mirrors of the reference interfaces (names, shapes, schedules,
registry) match the reference.  No device compute here."""
import os
import re

import numpy as np
import pytest
import torch

from prodiff_amd import FastDiff, GaussianDiffusion, WaveNet, _lib, synth
from prodiff_amd import schedules as S
from prodiff_amd import vocoder as V
from tests import golden_io as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    txt = open(os.path.join(ROOT, "include", "prodiff_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(pd_\w+|fd_\w+|nsf_\w+)\s*\(", txt, flags=re.M))


def test_library_exports_every_header_symbol():
    lib = _lib.lib()
    declared = header_functions()
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.pd_version() == 2
    assert lib.pd_build_config() == b"default"


def test_null_arguments_fail_loudly():
    lib = _lib.lib()
    rc = lib.pd_wavenet_forward(None, None, None, None, None, 1, 1, None, 0, None)
    assert rc == 1 and b"null" in lib.pd_last_error()
    assert lib.fd_sample(None, None, None, None, None, None, 4, None, None, 0, None, None, None, 1, 1, None, 0, None) == 1


def test_wavenet_state_dict_matches_reference_names():
    for (M, H, L, C, cyc) in [(80, 256, 20, 256, 1), (64, 256, 20, 256, 5), (80, 32, 4, 64, 2)]:
        net = WaveNet(M, H, L, C, cyc)
        ref = synth.wavenet_param_shapes(M, H, L, C)
        sd = net.state_dict()
        assert list(sd) == list(ref)
        assert all(tuple(sd[k].shape) == tuple(v) for k, v in ref.items())
        assert len(net.ordered_params()) == 6 + 8 * L + 4


def test_gaussian_diffusion_buffers_match_reference():
    d = G.load("prodiff_t2_m80")
    gd = GaussianDiffusion(80, WaveNet(80, 256, 20, 256, 1), timesteps=2, time_scale=1000, max_beta=40.0)
    bufs = {k: v for k, v in gd.state_dict().items() if not k.startswith("denoise_fn")}
    ref = G.prodiff_buffers(d)
    assert set(bufs) == set(ref)
    for k in ref:
        np.testing.assert_allclose(bufs[k].numpy(), ref[k], rtol=1e-6, err_msg=k)


def test_fastdiff_state_dict_matches_reference_names():
    m = FastDiff()
    ref = synth.fastdiff_param_shapes()
    sd = m.state_dict()
    assert set(sd) == set(ref)
    assert all(tuple(sd[k].shape) == tuple(v) for k, v in ref.items())
    m.remove_weight_norm()
    ref2 = synth.fastdiff_param_shapes(weight_norm=False)
    assert set(m.state_dict()) == set(ref2)
    assert len(m._convs_in_order()) * 2 == 2 + 4 + 30 * 3 + 8 * 3 + 2


def test_prodiff_schedules_match_reference():
    s = G.load("schedules")
    for ts in (1, 2, 4, 8, 100):
        for mb in (40.0, 0.06):
            betas = S.get_noise_schedule_list("vpsde", ts + 1, min_beta=0.1, max_beta=mb)
            for k, v in S.diffusion_buffers(betas).items():
                np.testing.assert_allclose(v, s[f"t{ts}_mb{mb}_{k}"], rtol=1e-6, atol=0, err_msg=k)


def test_prodiff_schedule_types_match_reference():
    """linear / cosine / logsnr (prodiff.py:27-46) at max_beta 0.06.  logsnr returns
    log-SNR values, not betas: the reference's buffers hold NaN/inf there, and so do ours."""
    s = G.load("schedules")
    for st in ("linear", "cosine", "logsnr"):
        for ts in (4, 100):
            betas = S.get_noise_schedule_list(st, ts + 1, min_beta=0.1, max_beta=0.06)
            with np.errstate(all="ignore"):
                bufs = S.diffusion_buffers(betas)
            for k, v in bufs.items():
                np.testing.assert_allclose(v, s[f"{st}_t{ts}_{k}"], rtol=1e-6, atol=0, equal_nan=True,
                                           err_msg=f"{st} t{ts} {k}")


def test_fastdiff_schedules_match_reference():
    s = G.load("schedules")
    at = S.fastdiff_train_alpha()
    np.testing.assert_array_equal(at, s["fd_train_alpha"])
    for n in (3, 4, 6, 8, 200, 1000):
        b, a, sg, st = S.fastdiff_infer_params(S.fastdiff_reverse_schedule(n), at)
        np.testing.assert_array_equal(b, s[f"fd_n{n}_beta"])
        np.testing.assert_allclose(a, s[f"fd_n{n}_alpha"], rtol=1e-6)
        np.testing.assert_allclose(sg, s[f"fd_n{n}_sigma"], rtol=1e-6)
        # steps map alpha into the 1000-entry training table by (alpha[t]-a)/(alpha[t]-alpha[t+1]),
        # which amplifies a 1-ulp alpha difference ~100x; the fixture ran torch's CPU sqrt, which
        # is not correctly rounded on 4 of the 1000-step entries (IEEE sqrt here and on the GPU,
        # where the reference keeps these tensors: fastdiff.py:60-63 `.cuda()`)
        np.testing.assert_allclose(st, s[f"fd_n{n}_steps"], atol=1e-4 if n < 200 else 2e-4)


def test_vocoder_registry():
    assert V.get_vocoder_cls("FastDiff") is V.FastDiff
    assert V.get_vocoder_cls("fastdiff") is V.FastDiff
    with pytest.raises(ValueError):
        V.get_vocoder_cls("nope")


def test_no_cpu_fallback_on_cpu_tensors():
    net = WaveNet(80, 32, 2, 64, 1)
    with pytest.raises(_lib.HipError):
        net(torch.zeros(1, 1, 80, 4), torch.zeros(1), torch.zeros(1, 32, 4))


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "prodiff_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith(".py"):
                src = open(os.path.join(dp, f)).read()
                assert "oracle" not in re.sub(r"#.*", "", src).replace('"""', ""), f


TEACHER_HP = dict(audio_num_mel_bins=128, hidden_size=256, enc_layers=4, enc_ffn_kernel_size=9, dropout=0.1,
                  num_heads=2, num_spk=3, languages=["zh", "jp"], residual_layers=20, residual_channels=256,
                  dilation_cycle_length=1, timesteps=4, timescale=1000, schedule_type="vpsde", max_beta=40.0,
                  spec_min=[-12], spec_max=[0], use_voicing_embed=True, use_breath_embed=True)


@pytest.mark.parametrize("gender", [False, True])
def test_teacher_state_dict_matches_reference_names(gender):
    """Key order/shapes of the condition stage == the reference teacher's (verified against
    the reference module by tests/golden/gen_golden.py:gen_cond), diffusion under `diffusion.`."""
    from prodiff_amd.teacher import ProDiffTeacher
    hp = dict(TEACHER_HP, use_gender_id=gender)
    t = ProDiffTeacher(40, hp)
    sd = t.state_dict()
    ref = synth.cond_param_shapes(40, num_langs=3, **{k: v for k, v in hp.items() if k != "num_langs"})
    cond_keys = [k for k in sd if not k.startswith("diffusion.") and k != "encoder.embed_positions._float_tensor"]
    assert cond_keys == list(ref)
    assert all(tuple(sd[k].shape) == tuple(v) for k, v in ref.items())
    assert "encoder.embed_positions._float_tensor" in sd
    assert list(k[len("diffusion.denoise_fn."):] for k in sd if k.startswith("diffusion.denoise_fn.")) == \
        list(synth.wavenet_param_shapes(128, 256, 20, 256))
    dims = t.cond_dims()
    assert _lib.lib().pd_cond_num_params(dims) == len(t.ordered_cond_params()) == len(ref)


def test_teacher_needs_gpu_and_lang_seq():
    from prodiff_amd.teacher import ProDiffTeacher
    t = ProDiffTeacher(40, TEACHER_HP)
    tok = torch.ones(1, 4, dtype=torch.long)
    m2p = torch.tensor([[1, 2, 3, 4]])
    with pytest.raises(AssertionError):
        t.forward_condition(tok, m2p, torch.zeros(1, 4), spk_embed_id=torch.zeros(1, dtype=torch.long))
    with pytest.raises(_lib.HipError):
        t.forward_condition(tok, m2p, torch.zeros(1, 4), lang_seq=tok, spk_embed_id=torch.zeros(1, dtype=torch.long),
                            voicing=torch.zeros(1, 4), breath=torch.zeros(1, 4))


def test_rel_pos_table_grows_like_the_reference():
    """RelPositionalEncoding's table (espnet_positional_embedding.py:24-45) starts at 5,000 rows,
    grows to a longer input's length and never shrinks; the mirror tracks the same length and
    hands it to the kernel as pd_cond_dims.rel_pos (0 when the encoder uses the sinusoid)."""
    from prodiff_amd.teacher import ProDiffTeacher
    t = ProDiffTeacher(40, dict(TEACHER_HP, rel_pos=True))
    assert t.cond_dims().rel_pos == 5000
    t.encoder.embed_positions.extend(4000)
    assert t.cond_dims().rel_pos == 5000
    t.encoder.embed_positions.extend(6001)
    t.encoder.embed_positions.extend(21)
    assert t.cond_dims().rel_pos == 6001
    assert ProDiffTeacher(40, TEACHER_HP).cond_dims().rel_pos == 0


def test_utt_ids_host_checks():
    with pytest.raises(_lib.HipError):
        _lib.utt_ids([1, 2], 3, "cpu")
    with pytest.raises(_lib.HipError):
        _lib.utt_ids([-1, 2], 2, "cpu")
    assert _lib.utt_ids(None, 3, "cpu") is None
    d = _lib.utt_ids([4, 5], 2, "cpu")
    assert d.dtype == torch.int32 and d.tolist() == [4, 5]


def test_cond_create_rejects_bad_dims():
    lib = _lib.lib()
    d = _lib.pd_cond_dims(40, 256, 4, 9, 3, 1, 3, 1, 1, 0, 1, 0, 0)   # 256 / 3 heads
    h = _lib.C.c_void_p()
    assert lib.pd_cond_create(_lib.C.byref(d), None, 0, None, _lib.C.byref(h)) != 0
    d = _lib.pd_cond_dims(40, 256, 4, 9, 2, 1, 0, 1, 1, 1, 0, 0, 0)   # gender without lang_embed
    assert lib.pd_cond_num_params(_lib.C.byref(d)) > 0


def test_bench_traffic_keyed_by_workload(tmp_path):
    """bench.py takes `roofline.traffic` only from a PMC summary of the same workload: a C4
    line (32 utterances per GPU) must not carry a C3 (8 per GPU) measurement."""
    import json
    import bench
    f = tmp_path / "r09_v1_traffic.json"
    # the current instantiation (r04 added the tiles-per-wave argument; a pattern that ended at
    # `false>` matched only round-3 summaries)
    sym = "void (anonymous namespace)::lvc_block_bf16_kernel<384, true, true, true, true, false, 2>((anonymous namespace)::LvcBlockArgs)"
    json.dump({"bench_tag": "fd_lvc_block_final", "config": "C3", "batch": 8, "frames": 861,
               "kernels": {sym: {"traffic_bytes_per_launch": 1.0e8, "launches": 4}}}, open(f, "w"))
    assert bench.pmc_traffic("fd_lvc_block_final", "C3", 8, 861, str(f))[0] == 1.0e8
    assert bench.pmc_traffic("fd_lvc_block_final", "C4", 32, 861, str(f)) == (None, None, None)
    assert bench.pmc_traffic("fd_lvc_block_final", "C3", 8, 100, str(f)) == (None, None, None)
    # legacy (pre-r03) summaries are C3 8 x 861 unless named *c5*
    assert bench.traffic_workload({}, "profiles/r02_v4_traffic.json") == ("C3", 8, 861)
    assert bench.traffic_workload({}, "profiles/r02_v4c5_traffic.json") == ("C5", 8, 861)
    # a C4 line reads only a C4 summary (profiles/r03_v4c4_traffic.json), never a C3 figure
    c3 = bench.pmc_traffic("fd_lvc_block_final", "C3", 8, 861)
    c4 = bench.pmc_traffic("fd_lvc_block_final", "C4", 32, 861)
    if c4[0] is not None:
        assert "c4" in c4[1] and c4[0] > 3 * c3[0]
    assert bench.pmc_traffic("fd_lvc_block_final", "C4", 16, 861) == (None, None, None)


def test_bench_tables_cover_every_dominant_tag():
    """bench.py refuses an untagged slowest kernel: the tags that lead C2 / C3 / C4 /
    C5 profiles -- the WaveNet stack, the fp32 layer launches, the LVC blocks, the kernel
    predictor, the NSF pair / upsample / noise convs -- all have FLOP and byte entries."""
    import bench
    fl = bench.flops_per_launch(8, 861, "bf16")
    by = bench.bytes_per_launch(8, 861, "bf16")
    sf, sb = bench.svs_tables(8, 861, 120, "bf16")
    fl.update(sf)
    by.update(sb)
    for tag in ("wn_stack", "wn_gate", "wn_resskip", "fd_lvc_block_final", "fd_kp_kernel", "fd_kp_hidden",
                "fd_lvc_block_ups", "fd_lvc_block_sub", "fd_dblock_fused", "nsf_pair", "nsf_pair16", "nsf_rb16", "nsf_res",
                "nsf_ups", "nsf_noise_conv", "nsf_source", "nsf_post"):
        assert tag in fl and tag in by and by[tag] > 0, tag
    # the stack's mean launch: 10 layers of 26.2 MFLOP per frame plus half the in/out projections
    per_frame = fl["wn_stack"] / (8 * 861)
    assert 10 * 2 * 2 * 256 * 1280 < per_frame < 10 * 2 * 2 * 256 * 1280 * 1.02
    # 24 pair launches + 1 nsf_rb32 launch (r06: the 32-channel taps-3 ResBlock whole) per C5 forward carry
    # all ResBlock FLOPs of the C = 128 / 64 / 32 stages
    F = 8 * 861
    pair_total = sum(2 * 2 * 3 * 21 * F * r * c * c for r, c in bench.nsf_stage_dims() if c in bench.NSF_PAIR_C)
    assert abs(fl["nsf_pair"] * 24 + fl["nsf_rb32"] - pair_total) < 1e-6 * pair_total
    # ... and 9 nsf_pair16 launches the C = 16 stage's (r05); no single 16-channel convs remain in bf16
    p16 = sum(2 * 2 * 3 * 21 * F * r * c * c for r, c in bench.nsf_stage_dims() if c in bench.NSF_PAIR16_C)
    assert abs(fl["nsf_pair16"] * 9 - p16) < 1e-6 * p16 and by["nsf_res_small"] == 0
    # ... or 3 nsf_rb16 launches (r06: one per whole ResBlock1, the default), the same FLOPs
    assert abs(fl["nsf_rb16"] * 3 - p16) < 1e-6 * p16 and by["nsf_rb16"] > 0
    with pytest.raises(SystemExit):
        bench.dominant_kernel({"mystery": (1, 5.0), "wn_stack": (2, 1.0)}, fl, by)
    assert bench.dominant_kernel({"nsf_pair": (27, 5.0), "wn_stack": (2, 1.0)}, fl, by) == "nsf_pair"


def test_golden_fixtures_in_parts(tmp_path):
    """golden_io.save cuts a fixture into files of at most PART_BYTES of arrays (an array larger
    than that along its flattened length) and load() returns the arrays bit for bit; no committed
    fixture file exceeds 1 MiB."""
    rng = np.random.default_rng(0)
    arrays = {"a": rng.standard_normal((3, 50, 7)).astype(np.float32), "n": np.int64(5), "names": np.array(["x", "yz"]),
              "b": rng.standard_normal(1001), "c": rng.integers(0, 9, (40,)), "empty": np.zeros((0, 4), np.float32)}
    paths = G.save("fx", arrays, root=str(tmp_path), part_bytes=2000)
    assert len(paths) > 3 and paths == G.part_paths("fx", str(tmp_path))
    for p in paths:
        with np.load(p) as z:
            assert sum(z[k].nbytes for k in z.files) <= 2000
    back = G.load("fx", root=str(tmp_path))
    assert set(back) == set(arrays)
    for k, v in arrays.items():
        assert back[k].dtype == np.asarray(v).dtype and back[k].shape == np.asarray(v).shape
        np.testing.assert_array_equal(back[k], v)
    # a smaller rewrite leaves no stale part behind
    assert G.save("fx", {"n": np.int64(1)}, root=str(tmp_path)) == G.part_paths("fx", str(tmp_path))
    big = [f for f in os.listdir(G.GOLDEN) if os.path.getsize(os.path.join(G.GOLDEN, f)) > 1 << 20]
    assert not big, big


def _bench_line(monkeypatch, capsys, argv):
    import json
    import bench
    monkeypatch.setattr("sys.argv", ["bench.py"] + argv)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    bench.main()
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_bench_dump_outputs_dry_run(tmp_path, monkeypatch, capsys):
    """`--dump-outputs DIR` writes the last timed step's outputs as float32 DIR/<name>.npy, the same
    from run to run; `--steps` sets the timed steps and the line carries `ms_per_step` (CPU dry run:
    stub synthesis, mel = the condition's first 80 columns, so the dump pins the inputs too)."""
    argv = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "2", "--frames", "7", "--dry-run"]
    runs = []
    for name in ("a", "b"):
        d = _bench_line(monkeypatch, capsys, argv + ["--dump-outputs", str(tmp_path / name)])
        assert d["steps"] == 3 and d["warmup"] == 1 and d["full"] is False
        assert d["ms_per_step"] > 0 and d["unit"] == "mel-frames/s" and d["higher_is_better"] is True
        assert abs(d["value"] - 2 * 7 * 1e3 / d["ms_per_step"]) <= 0.01 * d["value"]
        assert sorted(os.listdir(tmp_path / name)) == ["mel.npy", "wav.npy"]
        runs.append({k: np.load(tmp_path / name / (k + ".npy")) for k in ("mel", "wav")})
    for k, shape in (("mel", (2 * 7, 80)), ("wav", (2 * 7 * 256,))):
        assert runs[0][k].dtype == np.float32 and runs[0][k].shape == shape
        np.testing.assert_array_equal(runs[0][k], runs[1][k])
    assert np.abs(runs[0]["mel"]).max() > 0


def test_bench_dump_outputs_sample_is_fixed(tmp_path, monkeypatch):
    """Outputs over the byte budget are cut to a fixed sample: the same indices on every call, each
    array its share of the budget."""
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4000)
    g = torch.Generator().manual_seed(0)
    mels = [torch.randn(9, 80, generator=g) for _ in range(2)]
    wavs = [torch.randn(9 * 256, generator=g) for _ in range(2)]
    for name in ("a", "b"):
        bench.dump_outputs(str(tmp_path / name), (mels, wavs), True, False)
    a = {k: np.load(tmp_path / "a" / (k + ".npy")) for k in ("mel", "wav")}
    b = {k: np.load(tmp_path / "b" / (k + ".npy")) for k in ("mel", "wav")}
    assert 0 < a["mel"].nbytes + a["wav"].nbytes <= 4000 and a["wav"].size > a["mel"].size > 0
    for k, full in (("mel", torch.cat(mels)), ("wav", torch.cat(wavs))):
        np.testing.assert_array_equal(a[k], b[k])
        assert np.isin(a[k], full.numpy().reshape(-1)).all()
    bench.dump_outputs(str(tmp_path / "p"), torch.ones(2, 5, dtype=torch.float64), False, True)
    assert np.load(tmp_path / "p" / "pitch.npy").dtype == np.float32


def test_bench_full_option_off_by_default(monkeypatch, capsys):
    """`--full` is an option of every run and off by default; the plain line leaves the fields of the
    measurements behind it empty (CPU dry run: the launcher and the line, no GPU legs)."""
    argv = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "2", "--frames", "7", "--dry-run"]
    d = _bench_line(monkeypatch, capsys, argv)
    assert d["full"] is False
    assert d["cpu_baseline"] is None and d["cpu_baseline_port"] is None and d["utilisation"] is None
    assert d["roofline"] is None and d["kernels"] == {}
    assert _bench_line(monkeypatch, capsys, argv + ["--full"])["full"] is True


def test_collate_pad_stack_equals_per_item_pad():
    """pipeline._pad_stack (the batch collate: one stack for equal lengths, one zero fill and a copy
    per row otherwise) equals the per-item F.pad + stack it replaced, for float frames and integer
    tokens, ragged and equal lengths."""
    from prodiff_amd.pipeline import SvsSynthesizer, Synthesizer, _pad_stack

    def ref(items):
        n = max(int(v.shape[0]) for v in items)
        pad = [(0, 0) * (v.dim() - 1) + (0, n - int(v.shape[0])) for v in items]
        return torch.stack([torch.nn.functional.pad(v, p) for v, p in zip(items, pad)])

    g = torch.Generator().manual_seed(3)
    cases = [[torch.randn(t, 4, generator=g) for t in (5, 2, 4)],
             [torch.randn(3, 4, generator=g) for _ in range(3)],
             [torch.randint(0, 9, (t,), generator=g) for t in (4, 1, 4)],
             [torch.randn(1, 2, generator=g)]]
    for items in cases:
        out = _pad_stack(items)
        assert out.dtype == items[0].dtype
        assert torch.equal(out, ref(items))
    assert torch.equal(Synthesizer.collate(cases[0]), ref(cases[0]))
    b = SvsSynthesizer.collate([{"txt_tokens": torch.arange(1, 4), "mel2ph": torch.ones(5, dtype=torch.long)},
                                {"txt_tokens": torch.arange(1, 3), "mel2ph": torch.ones(2, dtype=torch.long)}])
    assert b["ntok"] == [3, 2] and b["nframes"] == [5, 2]
    assert b["txt_tokens"].tolist() == [[1, 2, 3], [1, 2, 0]]
    assert b["mel2ph"].tolist() == [[1] * 5, [1, 1, 0, 0, 0]]


# ---------------------------------------------------------------- the shared handle lifecycle
NSF_SMALL = dict(synth.NSF_DEFAULTS, upsample_initial_channel=32, upsample_rates=(4, 4), upsample_kernel_sizes=(8, 8))


def _four_modules():
    """One small instance of each module that owns a native handle, and the call that packs it."""
    from prodiff_amd.nsf_hifigan import Generator
    from prodiff_amd.teacher import ProDiffTeacher
    wn, fd, g, t = WaveNet(80, 32, 2, 64, 1), FastDiff(), Generator(NSF_SMALL), ProDiffTeacher(40, TEACHER_HP)
    return [("WaveNet", wn, wn.handle), ("FastDiff", fd, fd.handle), ("NSF-HiFiGAN", g, g.handle),
            ("ProDiffTeacher", t, t.cond_handle)]


def _four_creates():
    """(create function, dims struct, parameter count) of the four components, small valid dims."""
    from prodiff_amd.nsf_hifigan import Generator
    from prodiff_amd.teacher import ProDiffTeacher
    lib = _lib.lib()
    fd = _lib.fd_dims(1, 32, 80, 3, (_lib.C.c_int * 4)(8, 8, 4, 0), 4, 3, 64, 3, 128, 512, 512)
    nsf = Generator(NSF_SMALL)._dims()
    cond = ProDiffTeacher(40, TEACHER_HP).cond_dims()
    return [(lib.pd_wavenet_create, _lib.pd_wavenet_dims(80, 32, 2, 64, 1), 6 + 8 * 2 + 4),
            (lib.fd_create, fd, len(FastDiff()._convs_in_order()) * 2),
            (lib.nsf_create, nsf, lib.nsf_num_params(_lib.C.byref(nsf))),
            (lib.pd_cond_create, cond, lib.pd_cond_num_params(_lib.C.byref(cond)))]


def _call_create(create, dims, ptrs, dtype):
    out = _lib.C.c_void_p(0x5a5a)
    arr = (_lib.C.c_void_p * len(ptrs))(*ptrs)
    rc = create(_lib.C.byref(dims), arr, dtype, None, _lib.C.byref(out))
    return rc, _lib.lib().pd_last_error().decode(), out.value


@pytest.mark.skipif(torch.cuda.is_available(), reason="hands fake parameter pointers to the library: only where no device can read them")
@pytest.mark.parametrize("dtype", [_lib.PD_DTYPE_F32, _lib.PD_DTYPE_BF16])
def test_create_without_a_device_fails_cleanly(dtype):
    """Without a device every create stops at the weight pool's hipMalloc: PD_ERR_HIP, the pool's
    error text, the out handle untouched and no device bytes counted as live."""
    for create, dims, n in _four_creates():
        rc, msg, out = _call_create(create, dims, [0x1000 + 64 * i for i in range(n)], dtype)
        assert rc == 2 and "hipMalloc failed for" in msg and msg.endswith("weights"), (create.__name__, rc, msg)
        assert out == 0x5a5a
        assert _lib.lib().pd_live_device_bytes() == 0


def test_create_names_a_null_parameter():
    """A null entry in the parameter list is refused before anything is allocated or launched,
    by the same check in all four components: PD_ERR_ARG and the entry's index."""
    for create, dims, n in _four_creates():
        ptrs = [0x1000 + 64 * i for i in range(n)]
        ptrs[3] = None
        rc, msg, out = _call_create(create, dims, ptrs, _lib.PD_DTYPE_F32)
        assert rc == 1 and msg == "argument: null parameter 3", (create.__name__, rc, msg)
        assert out == 0x5a5a
        assert _lib.lib().pd_live_device_bytes() == 0


def test_unknown_options_and_dtypes_are_refused():
    for name, m, _ in _four_modules():
        with pytest.raises(ValueError):
            m.set_compute_dtype("fp16")
        assert m.set_compute_dtype("bf16") is m
        if hasattr(m, "set_options"):
            with pytest.raises(ValueError, match=f"unknown {name} option 'nope'"):
                m.set_options(nope=1)
            assert m.set_options() is m
    assert [hasattr(m, "set_options") for _, m, _ in _four_modules()] == [True, True, True, False]
    # the variants that lost their A/B runs are gone: their names are unknown, and the C setters answer their ids
    # as any unknown id and their values as any bad value.  No handle can be created without a device, so a zeroed
    # buffer, larger than either handle struct, stands in for one: the setters check the handle only for null and
    # refuse an id or value before they read or write it, so the buffer is never used as an object (were a
    # setter to accept one of these, it would return 0 and the assertion below would fail)
    _, fd, _ = _four_modules()[1]
    for k in ("kp_side", "lvc_ts_sub"):
        with pytest.raises(ValueError, match=f"option '{k}'"):
            fd.set_options(**{k: 1})
    L, h = _lib.lib(), _lib.C.create_string_buffer(1 << 16)
    for fn, option, values, text in ((L.fd_set_option, 1, (128, 256, 384), "unknown option 1"),
                                     (L.fd_set_option, 5, (0, 1), "unknown option 5"),
                                     (L.pd_wavenet_set_option, _lib.WN_OPTIONS["layer"], (1,), "PD_WN_OPT_LAYER")):
        for v in values:
            assert fn(h, option, v) == 1 and text in L.pd_last_error().decode(), (text, v)


def test_cpu_parameters_fail_loudly_in_handle():
    for name, m, handle in _four_modules():
        with pytest.raises(_lib.HipError, match=f"{name} parameters must live on the GPU"):
            handle()


class _StubHandle:
    """What HandleCache asks of a NativeHandle: get(signature, build, device) and close()."""

    def __init__(self):
        self.closed = 0

    def get(self, signature, build, device=None):
        self.signature, self.built, self.device = signature, build(), device
        return ("handle", signature)

    def close(self):
        self.closed += 1


def test_handle_cache_normalises_evicts_and_closes(monkeypatch):
    """_lib.HandleCache without a device: a CPU device is refused, two spellings of one device share an
    entry, the ninth key of a cache of eight closes exactly the oldest entry, close() closes the rest."""
    import contextlib
    monkeypatch.setattr(torch.cuda, "device", lambda device: contextlib.nullcontext())   # nothing to switch to here
    made = []

    def new():
        made.append(_StubHandle())
        return made[-1]

    cache = _lib.HandleCache("stub front end", "no_create", "no_destroy", limit=8)
    cache._new = new
    build = lambda device: (device, [])   # noqa: E731
    for cpu in ("cpu", torch.device("cpu")):
        with pytest.raises(_lib.HipError, match="stub front end.*no CPU fallback"):
            cache.get(cpu, (0.0, 1.0), build)
    assert not made and not cache.handles
    a = cache.get("cuda:0", (0.0, 1.0), build)
    assert cache.get(torch.device("cuda", 0), (0.0, 1.0), build) == a
    assert len(made) == 1 and list(cache.handles) == [(0.0, 1.0, "cuda:0")]
    assert made[0].built == (torch.device("cuda", 0), []) and made[0].device == torch.device("cuda", 0)
    assert made[0].signature == (0.0, 1.0, "cuda:0")
    cache.get("cuda:1", (0.0, 1.0), build)               # another device is another entry
    for k in range(2, 8):
        cache.get("cuda:0", (float(k), 1.0), build)
    assert len(cache.handles) == 8 and len(made) == 8 and not any(s.closed for s in made)
    cache.get("cuda:0", (8.0, 1.0), build)               # the ninth key
    assert len(cache.handles) == 8 and len(made) == 9
    assert [s.closed for s in made] == [1] + [0] * 8
    assert (0.0, 1.0, "cuda:0") not in cache.handles and (0.0, 1.0, "cuda:1") in cache.handles
    cache.close()
    assert [s.closed for s in made] == [1] * 9 and not cache.handles

    unlimited = _lib.HandleCache("stub front end", "no_create", "no_destroy")
    unlimited._new = new
    for k in range(12):
        unlimited.get("cuda:0", (k,), build)
    assert len(unlimited.handles) == 12 and not any(s.closed for s in made[9:])
