"""GPU tests of the pitch extractor's bf16 modes (pd_rmvpe_set_option PD_RMVPE_OPT_CONV_DTYPE / PD_RMVPE_OPT_GRU_DTYPE,
E2E0.set_compute_dtype) on the five cases of tests/rmvpe_cases.py and their committed fixtures.

Bars:
  fixture     native bf16 `hidden` and `feat` against the reference's f32 tensors under the project's bf16 bar
              (tests/bf16_bar.py: rel-L2 <= 1e-2, max-rel <= 2e-2), with both options and with each alone; every
              figure goes out on a BF16ERR line
  emulation   the native result against tests/rmvpe_bf16_emul.py's on the same input.  The two differ in the f32
              summation order and in the bf16 roundings of later inputs that this order flips, so the bar is what the
              order alone is worth in the emulation itself (tests/test_gpu_vr_bf16.py's header has the argument):
                  rel-L2(native, emulation) <= ORDER_FACTOR x order_noise(case),     ORDER_FACTOR = 1.5
              the ratio to rel-L2(emulation, fixture) is printed.  The order draws also evaluate the fp32 side that
              feeds a bf16 rounding (encoder.bn, the first conv, the pools) in f32 as its kernels state it: on the
              nine-conv rmvpe_shallow that, not the bf16 sums' order, is most of the distance (1.45e-4 of `feat`
              native against 2.8e-5 for the sums alone; tests/rmvpe_bf16_emul.py's header has the measurement)
  f0          on the two end-to-end clips of tests/test_gpu_rmvpe.py (0.5 s gliding tone, 16 and 44.1 kHz), against
              its float64 chain f0_chain64, in cents.  With the centre bin held at the fp32 native run's argmax the
              bar is 4 x the emulation's own largest error on that clip: the separation's native result sat up to
              about one rounding error from its emulation by summation order alone, 4 doubles that.  Free decode is
              compared on the frames whose float64 top-two margin is >= 4 x the emulation's largest |hidden| error
              (at least 0.4 of the frames), under the same bar.  On the synthetic fixtures free decode is not
              compared: their margins go down to 1e-5 and the emulation itself flips 2 % of rmvpe_full_b2t64's frames.
  the rest    bit-equality (torch.equal): fp32 untouched by a switch there and back, rows, batch position, 17 rows,
              graph replay and ragged rows in bf16; live bytes through the mirror's life
"""
import functools

import numpy as np
import pytest
import torch

import prodiff_amd
from prodiff_amd import _lib, synth
from prodiff_amd import rmvpe as RM
from tests import bf16_bar
from tests import rmvpe_bf16_emul as E
from tests import rmvpe_cases as RC
from tests import rmvpe_ref as R
from tests.test_gpu_rmvpe import case_net, cuda, extractor, f0_chain64, fixture, host_params
from tests.test_gpu_rmvpe_ragged import single_run

pytestmark = pytest.mark.gpu


def build_net(model_items, seed):
    model = dict(model_items)
    net = prodiff_amd.E2E0(model["n_blocks"], model["n_gru"], (2, 2), model["en_de_layers"], model["inter_layers"], 1,
                           model["en_out_channels"])
    net.load_state_dict({k: torch.from_numpy(v) for k, v in host_params(model_items, seed).items()})
    return net.cuda()


@functools.lru_cache(maxsize=None)
def bf16_net(model_items, seed, conv, gru):
    """One model per (architecture, seed, mode) for this module: the session's shared fp32 nets are never switched."""
    return build_net(model_items, seed).set_compute_dtype(conv, gru)


def case_bf16(name, conv="bf16", gru="bf16"):
    model, _, _, pseed, _ = RC.CASES[name]
    return bf16_net(tuple(sorted(model.items())), pseed, conv, gru)


def new_net(name):
    model, _, _, pseed, _ = RC.CASES[name]
    return build_net(tuple(sorted(model.items())), pseed)


@functools.lru_cache(maxsize=None)
def native(name, conv="bf16", gru="bf16"):
    hidden, feat = case_bf16(name, conv, gru).forward_features(cuda(fixture(name)["mel"]))
    return {"hidden": hidden.cpu().numpy(), "feat": feat.cpu().numpy()}


# ---------------------------------------------------------------- 1. against the fixture
MODES = [(name, "bf16", "bf16") for name in RC.CASES] + \
        [(name, c, g) for name in ("rmvpe_slim", "rmvpe_full_b2t64") for c, g in (("bf16", "fp32"), ("fp32", "bf16"))]


@pytest.mark.parametrize("name,conv,gru", MODES)
def test_bf16_meets_the_bars_against_the_fixture(name, conv, gru):
    d = fixture(name)
    got = native(name, conv, gru)
    for key in ("hidden", "feat"):
        assert got[key].shape == d[key].shape
        if key == "feat" and conv == "fp32":
            assert np.array_equal(got[key], case_net(name).forward_features(cuda(d["mel"]))[1].cpu().numpy())
        bf16_bar.assert_bf16_close(got[key], d[key], f"rmvpe {name} convs={conv} recurrence={gru} {key}")


# ---------------------------------------------------------------- 2. against the emulation
@pytest.mark.parametrize("name", list(RC.CASES))
def test_bf16_is_the_emulated_result_up_to_summation_order(name):
    d = fixture(name)
    emul = dict(zip(("feat", "hidden"), E.emulated(name)))
    noise = E.order_noise(name)
    got = native(name)
    ok = True
    for key in ("hidden", "feat"):
        r_emul = E.rel_l2(emul[key], d[key])
        r_nat = E.rel_l2(got[key], emul[key])
        bar = E.ORDER_FACTOR * noise[key]
        print(f"BF16ERR rmvpe {name} {key} rel-L2(native, emulation)={r_nat:.3e} rel-L2(emulation, fixture)={r_emul:.3e} "
              f"ratio={r_nat / r_emul:.3f} order noise of the emulation={noise[key]:.3e} bar={bar:.3e}", flush=True)
        assert r_emul > 1e-5                       # the emulation does round
        ok = ok and r_nat <= bar
    assert ok


# ---------------------------------------------------------------- 3. f0 from audio
@functools.lru_cache(maxsize=None)
def bf16_extractor():
    pe = RM.RMVPE({}, compute_dtype="bf16")
    pe.model.load_state_dict({k: torch.from_numpy(v) for k, v in
                              host_params(tuple(sorted(RC.FULL.items())), RC.CASES["rmvpe_full_b2t64"][3]).items()})
    pe.model.cuda()
    return pe


def mel64(audio, sr):
    """The network input of test_gpu_rmvpe.f0_chain64: float64 resampler and centred mel -> (mel [1, 128, T pad], T)"""
    from tests import resample_ref as RR
    x = np.asarray(audio, np.float64)[None]
    if sr != 16000:
        h, W, o, n = RR.table64(sr, 16000, lowpass_filter_width=128)
        x = RR.direct64(x, h.astype(np.float32).astype(np.float64), W, o, n)
    logmel = R.centered_mel(x, prodiff_amd.mel_filterbank(16000, 1024, 128, 30, 8000, htk=True))[2]
    T = logmel.shape[1]
    return np.pad(logmel, ((0, 0), (0, -T % 32), (0, 0))).transpose(0, 2, 1), T


def cents(a, b):
    return 1200.0 * np.abs(np.log2(np.asarray(a, np.float64) / np.asarray(b, np.float64)))


@pytest.mark.parametrize("sr", [16000, 44100])
def test_bf16_f0_from_audio(sr):
    audio = RC.harmonic_signal(sr, 0.5)
    f64, hidden64 = f0_chain64(audio, sr)
    mel, T = mel64(audio, sr)
    P = host_params(tuple(sorted(RC.FULL.items())), RC.CASES["rmvpe_full_b2t64"][3])
    emul = E.e2e0(P, RC.FULL, mel)[1][0, :T]
    wav = torch.from_numpy(audio)[None].cuda()
    h32 = extractor()._hidden_from_audio(wav, sr)
    hbf = bf16_extractor()._hidden_from_audio(wav, sr)
    assert hbf.shape == h32.shape == (1, T, RC.N_CLASS) and not torch.equal(hbf, h32)
    # the centre bin held at the fp32 native run's argmax
    center = h32.argmax(-1)
    c = center[0].cpu().numpy()
    f64c, femu = R.local_average_f0(hidden64, 0.03, c), R.local_average_f0(emul, 0.03, c)
    fnat = RM.to_local_average_f0(hbf, center=center, thred=0.03)[0].cpu().numpy()
    voiced = (f64c > 0) & (femu > 0) & (fnat > 0)
    assert voiced.any()
    e_emul, e_nat = float(cents(femu, f64c)[voiced].max()), float(cents(fnat, f64c)[voiced].max())
    bar = 4 * e_emul
    print(f"BF16ERR rmvpe f0 at {sr} Hz, centre fixed: {int(voiced.sum())} of {T} frames voiced, native {e_nat:.4f} cents, "
          f"emulation {e_emul:.4f} cents, bar {bar:.4f} cents", flush=True)
    # free decode, on the frames whose top-two margin stands clear of the mode's error
    err = float(np.abs(emul - hidden64).max())
    top = np.sort(hidden64, axis=-1)
    keep = top[:, -1] - top[:, -2] >= 4 * err
    ffree = RM.to_local_average_f0(hbf, thred=0.03)[0].cpu().numpy()
    both = keep & (f64 > 0) & (ffree > 0)
    e_free = float(cents(ffree, f64)[both].max()) if both.any() else float("nan")
    print(f"BF16ERR rmvpe f0 at {sr} Hz, free decode: emulation max|hidden error| {err:.3e}, {keep.mean():.2f} of the frames "
          f"kept, native {e_free:.4f} cents", flush=True)
    assert e_nat <= bar
    assert keep.mean() >= 0.4
    assert (hbf[0].argmax(-1).cpu().numpy()[keep] == hidden64.argmax(-1)[keep]).all()
    assert both.any()
    assert e_free <= bar


# ---------------------------------------------------------------- 4. fp32 untouched
@pytest.mark.parametrize("name", ["rmvpe_slim", "rmvpe_full_b2t64"])
def test_fp32_is_bit_equal_after_a_switch_there_and_back(name):
    mel = cuda(fixture(name)["mel"])
    h0, f0 = case_net(name).forward_features(mel)              # a net that never switched
    net = new_net(name)
    try:
        hb, fb = net.set_compute_dtype("bf16").forward_features(mel)
        h = net.handle().value
        h1, f1 = net.set_compute_dtype("fp32").forward_features(mel)
        assert net.handle().value == h                         # a switch flips the mode, it does not rebuild
        assert torch.equal(h1, h0) and torch.equal(f1, f0)
        assert not torch.equal(hb, h0) and not torch.equal(fb, f0)
        hb2, fb2 = case_bf16(name).forward_features(mel)
        assert torch.equal(hb, hb2) and torch.equal(fb, fb2)
        assert torch.equal(net.set_compute_dtype("bf16").forward_features(mel)[0], hb)
        # each option alone is its own result: the recurrence leaves feat alone, the convs do not
        hg, fg = net.set_compute_dtype("fp32", recurrence="bf16").forward_features(mel)
        assert torch.equal(fg, f0) and not torch.equal(hg, h0) and not torch.equal(hg, hb)
        hc, fc = net.set_compute_dtype("bf16", recurrence="fp32").forward_features(mel)
        assert torch.equal(fc, fb) and not torch.equal(hc, hb)
    finally:
        net.close()


# ---------------------------------------------------------------- 5. rows, position, blocks, graph and ragged in bf16
@pytest.mark.parametrize("name", ["rmvpe_slim", "rmvpe_full_b2t64"])
def test_bf16_rows_equal_their_single_runs(name):
    d = fixture(name)
    net = case_bf16(name)
    hidden, feat = net.forward_features(cuda(d["mel"]))
    for b in range(d["mel"].shape[0]):
        h1, f1 = net.forward_features(cuda(d["mel"][b:b + 1]))
        assert torch.equal(h1[0], hidden[b]) and torch.equal(f1[0], feat[b]), b


def test_a_bf16_row_does_not_depend_on_its_batch_position():
    d = fixture("rmvpe_slim")
    net = case_bf16("rmvpe_slim")
    alone = [net.forward_features(cuda(d["mel"][b:b + 1])) for b in range(2)]
    hidden, feat = net.forward_features(cuda(d["mel"][[0, 1, 0, 1, 0]]))
    for row, b in enumerate([0, 1, 0, 1, 0]):
        assert torch.equal(hidden[row], alone[b][0][0]) and torch.equal(feat[row], alone[b][1][0]), row


def test_bf16_more_rows_than_one_recurrence_block():
    """17 rows: the recurrence's second group of 16 batch rows holds a single row."""
    d = fixture("rmvpe_shallow")
    net = case_bf16("rmvpe_shallow")
    alone = [net.forward_features(cuda(d["mel"][b:b + 1])) for b in range(2)]
    order = [0, 1, 1, 0, 1] * 3 + [0, 1]
    hidden, feat = net.forward_features(cuda(d["mel"][order]))
    for row, b in enumerate(order):
        assert torch.equal(hidden[row], alone[b][0][0]) and torch.equal(feat[row], alone[b][1][0]), row


def test_bf16_graph_replay_equals_the_eager_call():
    d = fixture("rmvpe_slim")
    net = case_bf16("rmvpe_slim")
    mel = cuda(d["mel"]).transpose(1, 2).contiguous()
    eager = net.forward_time_major(mel).clone()
    assert not torch.equal(eager, case_net("rmvpe_slim").forward_time_major(mel))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = net.forward_time_major(mel)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_bf16_ragged_rows_equal_their_single_runs():
    """19 and 64 frames at 32 frames per unit: images 32 and 64 rows tall; NaN past every length."""
    frames = (19, 64)
    net = case_bf16("rmvpe_slim")
    mel = synth.synth_inputs(311, (2, 64, RC.N_MELS), loc=-4.0, scale=2.0)
    want = [single_run(net, mel[b], n, 32) for b, n in enumerate(frames)]
    want32 = [single_run(case_net("rmvpe_slim"), mel[b], n, 32) for b, n in enumerate(frames)]
    ragged = mel.copy()
    for b, n in enumerate(frames):
        ragged[b, n:] = np.nan
    hidden, feat = net.forward_time_major(cuda(ragged), return_feat=True, frames=list(frames))
    for b, n in enumerate(frames):
        assert not torch.isnan(hidden[b, :n]).any() and not torch.isnan(feat[b, :n]).any(), b
        assert torch.equal(hidden[b, :n], want[b][0]) and torch.equal(feat[b, :n], want[b][1]), b
        assert not torch.equal(want[b][0], want32[b][0]) and not torch.equal(want[b][1], want32[b][1]), b


# ---------------------------------------------------------------- 6. lifecycle
def test_bf16_mirror_lives_and_dies_with_the_handle():
    L = _lib.lib()
    name = "rmvpe_shallow"
    torch.cuda.synchronize()
    live = L.pd_live_device_bytes()
    net = new_net(name)
    mel = cuda(fixture(name)["mel"])
    y32 = net(mel)
    fp32_bytes = L.pd_live_device_bytes()
    assert fp32_bytes > live
    y = net.set_compute_dtype("bf16", recurrence="fp32")(mel)
    with_mirror = L.pd_live_device_bytes()
    assert with_mirror > fp32_bytes and not torch.equal(y, y32)
    yb = net.set_compute_dtype("bf16")(mel)                 # the second option finds the mirror standing
    assert L.pd_live_device_bytes() == with_mirror and not torch.equal(yb, y)
    assert torch.equal(yb, case_bf16(name)(mel))
    net.set_compute_dtype("fp32")(mel)
    net.set_compute_dtype("bf16")(mel)
    assert L.pd_live_device_bytes() == with_mirror          # later switches only flip the mode
    # a changed parameter repacks the pool and, the mode being applied to the new handle, its mirror
    with torch.no_grad():
        dict(net.named_parameters())["unet.encoder.layers.1.conv.0.conv.0.weight"].mul_(0.5)
    y2 = net(mel)
    assert not torch.equal(y2, yb) and L.pd_live_device_bytes() == with_mirror
    # through ctypes on the live handle: a bad option or value is PD_ERR_ARG and changes nothing
    h, st = net.handle(), _lib.stream_ptr(mel.device)
    assert L.pd_rmvpe_set_option(h, 2, _lib.PD_DTYPE_BF16, st) == 1
    assert L.pd_rmvpe_set_option(h, -1, _lib.PD_DTYPE_F32, st) == 1
    for opt in (_lib.PD_RMVPE_OPT_CONV_DTYPE, _lib.PD_RMVPE_OPT_GRU_DTYPE):
        assert L.pd_rmvpe_set_option(h, opt, 2, st) == 1
        assert L.pd_rmvpe_set_option(h, opt, -1, st) == 1
        assert L.pd_rmvpe_set_option(h, opt, _lib.PD_DTYPE_BF16, st) == 0
    assert torch.equal(net(mel), y2) and L.pd_live_device_bytes() == with_mirror
    net.close()
    assert L.pd_live_device_bytes() == live
