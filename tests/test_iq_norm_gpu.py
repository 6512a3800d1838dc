"""mdc_iq_u8_windows_norm / mdc_predict_host_iq_u8_norm / VTCNN2.predict_iq_u8(normalize="rms") on the MI355X, on inputs
for which tests/iq_norm_ref.py (numpy, int64 / float64) alone defines the answer.

  1. the four statistics are EXACTLY the reference's, at hops {128, 64, 16, 1, 37} and n up to 65,539, from a base pointer 2
     bytes into a larger buffer, with all-0, all-255, constant and single-pair windows; stats-only and frames + stats agree;
  2. every frame element within 2^-21 relative of the f64 reference, exactly 0 where a == 0 or E == 0, nothing non-finite.
     The bound is derived, not measured: a is exact; what remains is the conversion (float)E (<= 0.5 ulp), the square root
     (half its input's error + 0.5), one division (0.5), one multiplication (0.5) and the reference's own rounding to f32
     (0.5): under 4.5 units of 2^-24 with correctly rounded operations; 8 units = 2^-21;
  3. a per-channel byte offset changes neither the frames nor E under MDC_IQ_REMOVE_DC (bit-identical);
  4. predict_iq_u8(normalize="rms") == the two device calls by hand == the host driver at any chunk, bit for bit, for the
     bundled deployed nets, cnn.py's net and VT-CNN2; squelch labels exactly the reference's windows; normalize=None is the
     parent's path;
  5. on a TRAINED VT-CNN2: labels against the f64 oracle on the reference-normalised frames at test_trained_vtcnn2_gpu's
     floors, and accuracy at SNR >= 10 dB within the quantisation loss (measured on the oracle alone) of the float frames';
  6. the two calls are capturable in a hipGraph and replay bit-identically."""
import ctypes as C
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import iq_norm_ref as R                                                                  # noqa: E402
from conftest import GOLDEN, H5_NAMES                                                    # noqa: E402
from modulationdetectioncnn_amd import VTCNN2, Topology, _cabi, frontend                 # noqa: E402

REL = 2.0 ** -21
HOPS = [128, 64, 16, 1, 37]
COUNTS = [0, 1, 7, 255, 4097, 65536 + 3]
DC = _cabi.IQ_REMOVE_DC


def _capture(n, hop, seed):
    """2 bytes of padding + the bytes n windows read: random, with special windows at window indices 0, W, 2W, ... (W windows
    apart so that they do not overlap): all 0, all 255, constant I / constant Q, one non-zero pair, one pair off a constant."""
    nbytes = 2 * (hop * (n - 1) + 128) if n else 0
    buf = np.random.default_rng(seed).integers(0, 256, size=nbytes + 2, dtype=np.uint8)
    body = buf[2:]
    W = -(-128 // hop)
    special = [np.zeros(256, np.uint8), np.full(256, 255, np.uint8), np.tile(np.array([3, 250], np.uint8), 128),
               np.zeros(256, np.uint8), np.tile(np.array([128, 127], np.uint8), 128)]
    special[3][100:102] = (200, 7)
    special[4][30:32] = (129, 126)
    for j, seg in enumerate(special):
        if j * W < n:
            body[2 * hop * j * W: 2 * hop * j * W + 256] = seg
    return buf


def _run(dev_bytes, n, hop, level, flags, frames, stats):
    """mdc_iq_u8_windows_norm straight through the binding; dev_bytes: the uint8 device tensor whose data_ptr is window 0."""
    x = torch.full((n, 2, 128), float("nan"), dtype=torch.float32, device="cuda") if frames else None
    st = torch.full((n, 4), -1, dtype=torch.int32, device="cuda") if stats else None
    _cabi.check(_cabi.lib().mdc_iq_u8_windows_norm(dev_bytes.data_ptr() if n else None, n, hop, level, flags,
                                                   x.data_ptr() if frames and n else (0x1000 if frames else None),
                                                   st.data_ptr() if stats and n else (0x1000 if stats else None),
                                                   torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return (x.cpu().numpy() if frames else None), (frontend.stats_tensor_to_numpy(st) if stats else None)


def _check_frames(x, iq, n, hop, level, remove_dc):
    x64 = R.frames(iq, level, hop, remove_dc, n)
    assert np.isfinite(x).all()
    err = np.abs(x.astype(np.float64) - x64)
    worst = float((err / np.where(x64 != 0, np.abs(x64), 1.0)).max()) if n else 0.0
    print(f"hop {hop} n {n} level {level} dc {remove_dc}: largest relative error {worst / 2.0 ** -24:.3f} x 2^-24")
    assert (err <= REL * np.abs(x64)).all(), worst
    zero = (R.centred(iq, hop, remove_dc, n) == 0) | (R.stats(iq, hop, remove_dc, n)["energy"] == 0)[:, None, None]
    assert (x[zero] == 0).all()


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("hop", HOPS)
def test_stats_are_exact_and_frames_within_the_derived_bound(hop, n):
    buf = _capture(n, hop, seed=1000 * hop + n % 997)
    iq = buf[2:]
    dev = torch.from_numpy(buf).cuda()[2:]
    assert n == 0 or dev.data_ptr() % 4 == 2
    want = R.stats_records(iq, hop, True, n)
    _, only = _run(dev, n, hop, 7.8e-3, DC, False, True)
    x, both = _run(dev, n, hop, 7.8e-3, DC, True, True)
    for got in (only, both):
        assert got.shape == (n,)
        for k in R.STATS_DTYPE.names:
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    x_alone, _ = _run(dev, n, hop, 7.8e-3, DC, True, False)
    np.testing.assert_array_equal(x_alone.view(np.uint32), x.view(np.uint32))
    _check_frames(x, iq, n, hop, 7.8e-3, True)
    W = -(-128 // hop)
    if n > 3 * W:      # windows 0, W, 2W, 3W are the special segments themselves
        assert not x[0].any() and not x[W].any() and not x[2 * W].any()          # all 0, all 255, constant: E == 0
        assert both["energy"][0] == 0 and both["energy"][W] == 0 and both["energy"][2 * W] == 0 and both["energy"][3 * W] > 0


@pytest.mark.parametrize("level", [7.8e-3, 1.0, 3.0e4, 1.0e-30])
@pytest.mark.parametrize("remove_dc", [True, False])
@pytest.mark.parametrize("hop", [128, 37])
def test_frames_without_dc_removal_and_at_other_levels(hop, remove_dc, level):
    n = 4097
    buf = _capture(n, hop, seed=77)
    dev = torch.from_numpy(buf).cuda()[2:]
    x, st = _run(dev, n, hop, level, DC if remove_dc else 0, True, True)
    want = R.stats_records(buf[2:], hop, remove_dc, n)
    for k in R.STATS_DTYPE.names:
        np.testing.assert_array_equal(st[k], want[k], err_msg=k)
    _check_frames(x, buf[2:], n, hop, level, remove_dc)
    if not remove_dc:
        assert (st["energy"] >= 128 * 256).all() and x.any(axis=(1, 2)).all()      # s is odd: no window is empty without DC removal


def test_frontend_functions_and_power():
    hop, n = 16, 3000
    buf = _capture(n, hop, seed=9)[2:]
    st = frontend.window_stats_iq_u8(buf, hop=hop)
    want = R.stats_records(buf, hop, True, n)
    assert st.dtype == _cabi.IQ_WINDOW_STATS
    np.testing.assert_array_equal(st, want)
    np.testing.assert_array_equal(frontend.window_power_dbfs(st), R.power_dbfs(want["energy"].astype(np.int64)))
    x, st_dev = frontend.normalized_frames_from_iq_u8(buf, level=0.5, hop=hop, return_stats=True)
    assert x.shape == (n, 2, 128) and x.is_cuda
    np.testing.assert_array_equal(frontend.stats_tensor_to_numpy(st_dev), want)
    _check_frames(x.cpu().numpy(), buf, n, hop, 0.5, True)
    rms = torch.sqrt((x.double() ** 2).sum(dim=(1, 2)) / 128).cpu().numpy()
    live = want["energy"] > 0
    assert np.abs(rms[live] / 0.5 - 1).max() < 1e-6 and not rms[~live].any()
    x2 = frontend.normalized_frames_from_iq_u8(torch.from_numpy(buf).cuda(), level=0.5, hop=hop, remove_dc=False)
    _check_frames(x2.cpu().numpy(), buf, n, hop, 0.5, False)


@pytest.mark.parametrize("hop", [128, 16, 37])
def test_dc_offset_changes_nothing_under_remove_dc(hop):
    n = 5000
    iq = np.random.default_rng(hop).integers(35, 215, size=2 * (hop * (n - 1) + 128), dtype=np.uint8)
    shifted = iq.reshape(-1, 2).copy()
    shifted[:, 0] += 23
    shifted[:, 1] -= 31
    shifted = shifted.reshape(-1)
    xa, sa = _run(torch.from_numpy(iq).cuda(), n, hop, 7.8e-3, DC, True, True)
    xb, sb = _run(torch.from_numpy(shifted).cuda(), n, hop, 7.8e-3, DC, True, True)
    np.testing.assert_array_equal(xa.view(np.uint32), xb.view(np.uint32))
    np.testing.assert_array_equal(sa["energy"], sb["energy"])
    np.testing.assert_array_equal(sb["sum_i"].astype(np.int64) - sa["sum_i"], 2 * 128 * 23)
    np.testing.assert_array_equal(sb["sum_q"].astype(np.int64) - sa["sum_q"], -2 * 128 * 31)
    assert not np.array_equal(sa["sum_sq"], sb["sum_sq"])


# ---------------------------------------------------------------------------------------------------------------- composition
NETS = [("dep3", "f32"), ("dep3", "bf16"), ("dep10", "f32"), ("dep10", "bf16"), ("cnnpy", "f32"), ("vtcnn2", "f32"), ("vtcnn2", "bf16"),
        ("vtcnn2", "fp8")]


def _net(name, dtype):
    if name.startswith("dep"):
        for h5 in H5_NAMES:
            m = VTCNN2.from_npz(os.path.join(GOLDEN, "weights", h5 + ".npz"), dtype=dtype)
            if m.topology.filters == int(name[3:]):
                return m
        raise AssertionError(f"no bundled net with {name[3:]} filters")
    return VTCNN2.synthetic(Topology.vtcnn2(11) if name == "vtcnn2" else name, seed=2016, dtype=dtype)


def _varied_capture(n, hop, seed):
    """Random-walk-free but level-varied bytes: blocks of 4 KiB with amplitudes from 1 to 120 LSB around a drifting midpoint,
    so that window powers spread over tens of dB."""
    rng = np.random.default_rng(seed)
    nbytes = 2 * (hop * (n - 1) + 128)
    amp = np.repeat(rng.choice([1, 2, 4, 9, 20, 45, 120], size=nbytes // 4096 + 1), 4096)[:nbytes]
    mid = np.repeat(rng.integers(122, 134, size=nbytes // 4096 + 1), 4096)[:nbytes]
    return np.clip(np.rint(mid + amp * rng.standard_normal(nbytes) / 3), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("hop", [128, 16])
@pytest.mark.parametrize("name,dtype", NETS)
def test_normalised_predict_equals_the_two_calls_and_the_host_driver(name, dtype, hop):
    n = 2500
    m = _net(name, dtype)
    Cn = m.topology.classes
    iq = _varied_capture(n, hop, seed=31 + hop)
    dev = torch.from_numpy(iq).cuda()
    level = 7.8e-3
    # by hand: mdc_iq_u8_windows_norm, then forward_device
    x, st = frontend.normalized_frames_from_iq_u8(dev, level=level, hop=hop, return_stats=True)
    p_hand, l_hand, _ = m.forward_device(x)
    power_ref = R.power_dbfs(R.stats(iq, hop, True, n)["energy"])
    thr = float(np.median(power_ref))
    squelched = power_ref < thr
    assert 0 < squelched.sum() < n
    # device tensor in: chunked (batch_size) and whole
    for bs in (0, 700):
        p, l, pw = m.predict_iq_u8(dev, hop=hop, normalize="rms", level=level, batch_size=bs, return_power=True)
        assert torch.equal(p, p_hand) and torch.equal(l, l_hand), (name, dtype, hop, bs)
        np.testing.assert_allclose(pw.cpu().numpy(), power_ref, rtol=0, atol=1e-9)
    p, l = m.predict_iq_u8(dev, hop=hop, normalize="rms", level=level, squelch_dbfs=thr)
    assert torch.equal(p, p_hand)
    np.testing.assert_array_equal(l.cpu().numpy(), np.where(squelched, -1, l_hand.cpu().numpy()))
    # numpy in: the host driver, through the mirror ...
    p, l, pw = m.predict_iq_u8(iq, hop=hop, normalize="rms", level=level, squelch_dbfs=thr, return_power=True)
    np.testing.assert_array_equal(p.view(np.uint32), p_hand.cpu().numpy().view(np.uint32))
    np.testing.assert_array_equal(l, np.where(squelched, -1, l_hand.cpu().numpy()))
    np.testing.assert_array_equal(pw, power_ref)
    # ... and straight through the ABI at chunk sizes {default, 1,000, n}, with and without the statistics
    L, h = m._lib(), m._engine()
    want_st = R.stats_records(iq, hop, True, n)
    np.testing.assert_array_equal(frontend.stats_tensor_to_numpy(st), want_st)
    for chunk in (0, 1000, n):
        for with_stats in (True, False):
            probs, labels = np.full((n, Cn), np.nan, np.float32), np.full((n,), -7, np.int32)
            stats = np.zeros((n,), _cabi.IQ_WINDOW_STATS)
            m._check(L.mdc_predict_host_iq_u8_norm(h, iq.ctypes.data, n, hop, level, DC, probs.ctypes.data, labels.ctypes.data,
                                                   stats.ctypes.data if with_stats else None, chunk))
            np.testing.assert_array_equal(probs.view(np.uint32), p_hand.cpu().numpy().view(np.uint32), err_msg=str(chunk))
            np.testing.assert_array_equal(labels, l_hand.cpu().numpy())
            if with_stats:
                np.testing.assert_array_equal(stats, want_st)


@pytest.mark.parametrize("name,dtype", NETS)
def test_normalize_none_is_the_parents_path(name, dtype):
    n, hop = 1500, 16
    m = _net(name, dtype)
    iq = _varied_capture(n, hop, seed=5)
    dev = torch.from_numpy(iq).cuda()
    scale = 0.02 / 127.5
    p, l = m.predict_iq_u8(dev, scale, hop=hop, normalize=None)
    if name == "cnnpy":
        p_ref, l_ref, _ = m.forward_device(frontend.frames_from_iq_u8(dev, scale, hop=hop))
    else:
        p_ref = torch.empty((n, m.topology.classes), dtype=torch.float32, device="cuda")
        l_ref = torch.empty((n,), dtype=torch.int32, device="cuda")
        ws, ws_bytes = m._workspace(n)
        m._check(m._lib().mdc_forward_iq_u8(m._engine(), dev.data_ptr(), n, hop, scale, p_ref.data_ptr(), l_ref.data_ptr(),
                                            ws.data_ptr() if ws is not None else None, ws_bytes, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(p, p_ref) and torch.equal(l, l_ref)
    p_np, l_np = m.predict_iq_u8(iq, scale, hop=hop)
    np.testing.assert_array_equal(p_np.view(np.uint32), p_ref.cpu().numpy().view(np.uint32))
    np.testing.assert_array_equal(l_np, l_ref.cpu().numpy())


def test_host_driver_refuses_device_memory_and_frees_with_the_model():
    m = _net("dep3", "f32")
    dev = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    out = np.empty((16, 3), np.float32)
    rc = m._lib().mdc_predict_host_iq_u8_norm(m._engine(), dev.data_ptr(), 16, 128, 1.0, DC, out.ctypes.data, None, None, 0)
    assert rc == -22 and b"device memory" in m._lib().mdc_last_error()
    p, l = m.predict_iq_u8(np.zeros(4096, np.uint8), normalize="rms")          # constant windows: zero frames, finite rows
    assert np.isfinite(p).all() and p.shape == (16, 3)
    m._release()                                                                 # mdc_destroy frees the frame / statistics slots


# ---------------------------------------------------------------------------------------------------------------- graph capture
@pytest.mark.parametrize("name,dtype", [("dep3", "f32"), ("vtcnn2", "bf16"), ("cnnpy", "f32")])
def test_norm_and_forward_are_capturable(name, dtype):
    n, hop = 600, 16
    m = _net(name, dtype)
    dev = torch.from_numpy(_varied_capture(n, hop, seed=1)).cuda()
    p0, l0, w0 = m.predict_iq_u8(dev, hop=hop, normalize="rms", return_power=True)      # warm: workspace, code objects
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        p1, l1, w1 = m.predict_iq_u8(dev, hop=hop, normalize="rms", return_power=True)
    for seed in (2, 3):
        dev.copy_(torch.from_numpy(_varied_capture(n, hop, seed=seed)).cuda())          # same buffer, new capture
        p1.zero_()
        l1.fill_(-5)
        g.replay()
        torch.cuda.synchronize()
        pe, le, we = m.predict_iq_u8(dev, hop=hop, normalize="rms", return_power=True)
        torch.cuda.synchronize()
        assert torch.equal(p1, pe) and torch.equal(l1, le) and torch.equal(w1, we), (name, dtype, seed)


# ---------------------------------------------------------------------------------------------------------------- trained net
AMPLITUDES = [12, 50, 120]      # largest |byte - 127.5| of the quantised batch, LSB
DC_LSB = (3, -2)


def _trained_record():
    """Everything test 5 compares, computed once per process.  The f64 oracle only: held-out float frames, and the same
    frames quantised to bytes at each amplitude (+ DC) and normalised by the reference."""
    import trained_vtcnn2 as T
    from oracle import oracle_np as O
    if "iq_norm" not in T._cache:
        w, _ = T.trained()
        x, lab, snr, ref = T.held_out()
        hi = snr >= 10
        rec = {"weights": w, "labels": lab, "snr": snr, "hi": hi, "n_hi": int(hi.sum()),
               "oracle_float_acc_hi": float((ref["labels"] == lab)[hi].mean()), "amp": {}}
        for amp in AMPLITUDES:
            iq = R.quantise_frames(x, amp, DC_LSB)
            xn = R.frames(iq, 7.8e-3, 128, True)
            o = O.forward("vtcnn2", xn, w, dtype=np.float64)
            rec["amp"][amp] = {"iq": iq, "oracle_labels": o["labels"], "oracle_acc_hi": float((o["labels"] == lab)[hi].mean())}
        T._cache["iq_norm"] = rec
    return T._cache["iq_norm"]


def _vt(w, mode):
    m = VTCNN2(Topology.vtcnn2(11), dtype="fp8" if mode.startswith("fp8") else mode, fp8_bf16_features=mode == "fp8+bf16feat")
    m.set_weights(w)
    return m


def accuracy_record():
    """profiles/iq_norm_accuracy.json (tools/measure_iq_norm_accuracy.py writes what this returns): accuracy at SNR >= 10 dB
    versus amplitude for normalize="rms" and for the plain scale = 1/127.5 path, per dtype, and the oracle-only margin."""
    rec = _trained_record()
    lab, hi, n_hi = rec["labels"], rec["hi"], rec["n_hi"]
    p0 = rec["oracle_float_acc_hi"]
    out = {"frames": int(lab.size), "frames_snr_ge_10": n_hi, "dc_lsb": list(DC_LSB), "oracle_float_accuracy_snr_ge_10": p0,
           "binomial_3_sigma": 3.0 * float(np.sqrt(p0 * (1.0 - p0) / n_hi)), "amplitudes": {}}
    for amp in AMPLITUDES:
        a = rec["amp"][amp]
        row = {"oracle_normalised_accuracy_snr_ge_10": a["oracle_acc_hi"], "margin_quantisation_loss": max(0.0, p0 - a["oracle_acc_hi"])}
        for mode in ("f32", "bf16", "fp8"):
            m = _vt(rec["weights"], mode)
            row[f"{mode}_normalize_rms"] = float((m.predict_iq_u8(a["iq"], normalize="rms")[1] == lab)[hi].mean())
            row[f"{mode}_plain_scale"] = float((m.predict_iq_u8(a["iq"])[1] == lab)[hi].mean())
        out["amplitudes"][str(amp)] = row
    return out


@pytest.mark.parametrize("mode,floor", [("f32", 0.9995), ("bf16", 0.998), ("fp8", 0.985), ("fp8+bf16feat", 0.985)])
@pytest.mark.parametrize("amp", AMPLITUDES)
def test_trained_net_labels_against_the_oracle_on_the_normalised_frames(amp, mode, floor):
    """The floors are test_trained_vtcnn2_gpu.test_label_floor_against_the_oracle's (test_label_agreement_gpu.MODES + f32)."""
    from test_label_agreement_gpu import MODES
    assert dict(MODES + [("f32", 0.9995)])[mode] == floor
    rec = _trained_record()
    a = rec["amp"][amp]
    m = _vt(rec["weights"], mode)
    lab_dev = m.predict_iq_u8(torch.from_numpy(a["iq"]).cuda(), normalize="rms")[1].cpu().numpy()
    lab_host = m.predict_iq_u8(a["iq"], normalize="rms")[1]
    np.testing.assert_array_equal(lab_dev, lab_host)
    agree = float((lab_dev == a["oracle_labels"]).mean())
    print(f"amplitude {amp} LSB, {mode}: {agree:.5f} of labels equal the f64 oracle's on the normalised frames (floor {floor})")
    assert agree >= floor, agree


@pytest.mark.parametrize("mode", ["f32", "bf16", "fp8"])
@pytest.mark.parametrize("amp", AMPLITUDES)
def test_trained_net_accuracy_within_the_quantisation_loss(amp, mode):
    """Accuracy at SNR >= 10 dB of the normalised path >= the oracle's on the original float frames - margin, margin = the
    oracle's OWN loss from quantising + normalising those frames (f64, no kernel involved) + the binomial 3 sigma of the sample."""
    rec = _trained_record()
    a = rec["amp"][amp]
    p0, n_hi = rec["oracle_float_acc_hi"], rec["n_hi"]
    margin = max(0.0, p0 - a["oracle_acc_hi"]) + 3.0 * float(np.sqrt(p0 * (1.0 - p0) / n_hi))
    got = float((_vt(rec["weights"], mode).predict_iq_u8(a["iq"], normalize="rms")[1] == rec["labels"])[rec["hi"]].mean())
    print(f"amplitude {amp} LSB, {mode}: accuracy {got:.4f}; oracle on float frames {p0:.4f}, on normalised bytes {a['oracle_acc_hi']:.4f}; margin {margin:.4f}")
    assert got >= p0 - margin, (got, p0, margin)
