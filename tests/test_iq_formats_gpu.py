"""mdc_iq_windows / mdc_iq_windows_norm / mdc_predict_host_iq(_norm) / VTCNN2.predict_iq on the MI355X for signed 8- and 16-bit
captures, on inputs for which tests/iq_formats_ref.py (numpy, int64 / float64) alone defines the answer.

  1. the four 64-bit statistics are EXACTLY the reference's, at hops {128, 64, 1, 37} and n in {0, 1, 2, 7, 9, 255, 4097}, from a
     base pointer one pair into a larger buffer, with the windows planted where 32-bit arithmetic would wrap (all minimum:
     sum_sq = 2^38 and E = 0 under DC removal; alternating minimum / maximum: the largest E; ...); stats-only, frames + stats
     and frames-only runs agree bit for bit; one stats-only run past grid cap x windows per work-group (the stride loop);
  2. every frame element within 2^-21 relative of the f64 reference, exactly 0 where a == 0 or E == 0, nothing non-finite, with
     and without DC removal at levels {7.8e-3, 1, 3e4}.  The bound is derived as tests/test_iq_norm_gpu.py derives it: 128 s - c
     is exact (below 2^23); what remains is the conversion (float)E (<= 0.5 ulp; E has up to 46 bits here), the square root
     (half its input's error + 0.5), one division (0.5), one multiplication (0.5) and the reference's own rounding to f32
     (0.5): under 4.5 units of 2^-24 with correctly rounded operations; 8 units = 2^-21;
  3. identities that follow from power-of-two scaling of the defined chain, bit for bit: u8 bytes XOR 0x80 read as CI8 against
     the existing u8 kernel; CI8 << 8 read as CI16; MDC_IQ_CU8 through the new entries against the old ones; a DC offset;
  4. mdc_iq_windows == float32(s) * float32(scale) bit for bit;
  5. predict_iq(normalize="rms") == the two device calls by hand == the host driver at any chunk, bit for bit, for the bundled
     deployed nets, cnn.py's net and VT-CNN2; squelch labels exactly the reference's windows; normalize=None is
     mdc_iq_windows + forward; "cu8" is predict_iq_u8;
  6. windows-norm + forward replay bit-identically from a captured graph;
  7. on a TRAINED VT-CNN2: labels against the f64 oracle on the reference-normalised frames at test_label_agreement_gpu's floors."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import iq_formats_ref as R                                                               # noqa: E402
from conftest import GOLDEN, H5_NAMES                                                    # noqa: E402
from modulationdetectioncnn_amd import VTCNN2, Topology, _cabi, frontend                 # noqa: E402

REL = 2.0 ** -21
DC = _cabi.IQ_REMOVE_DC
FMT = {"cu8": _cabi.IQ_CU8, "ci8": _cabi.IQ_CI8, "ci16": _cabi.IQ_CI16}
GRID_CAP_WINDOWS = 16384 * 8          # iq_formats.hip: kFmtGridCap work-groups x 2 * kFmtWaves windows


def _specials(fmt):
    """256-sample windows: all minimum, all maximum, alternating minimum / maximum pairs, I minimum with Q maximum, all zero, one
    non-zero pair, one sample one LSB off a constant."""
    lo, hi, dt = R.SAMPLE_MIN[fmt], R.SAMPLE_MAX[fmt], R.DTYPE[fmt]
    alt = np.empty(256, dt)
    alt[0::4], alt[1::4], alt[2::4], alt[3::4] = lo, lo, hi, hi
    one = np.zeros(256, dt)
    one[100:102] = (hi, lo // 3)
    off = np.tile(np.array([hi // 2, lo // 5], dt), 128)
    off[31] += 1
    return [np.full(256, lo, dt), np.full(256, hi, dt), alt, np.tile(np.array([lo, hi], dt), 128), np.zeros(256, dt), one, off]


def _capture(fmt, n, hop, seed):
    """One pair of padding + the samples n windows read: random over the whole range, with the special windows at window indices
    0, W, 2W, ... (W windows apart so that they do not overlap)."""
    nsamples = 2 * (hop * (n - 1) + 128) if n else 0
    buf = np.random.default_rng(seed).integers(R.SAMPLE_MIN[fmt], R.SAMPLE_MAX[fmt] + 1, size=nsamples + 2).astype(R.DTYPE[fmt])
    body = buf[2:]
    W = -(-128 // hop)
    for j, seg in enumerate(_specials(fmt)):
        if j * W < n:
            body[2 * hop * j * W: 2 * hop * j * W + 256] = seg
    return buf


def _run(dev, fmt, n, hop, level, flags, frames, stats):
    """mdc_iq_windows_norm straight through the binding; dev: the device tensor whose data_ptr is window 0."""
    x = torch.full((n, 2, 128), float("nan"), dtype=torch.float32, device="cuda") if frames else None
    st = torch.full((n, 4), -1, dtype=torch.int64, device="cuda") if stats else None
    _cabi.check(_cabi.lib().mdc_iq_windows_norm(dev.data_ptr() if n else None, FMT[fmt], n, hop, level, flags,
                                                x.data_ptr() if frames and n else (0x1000 if frames else None),
                                                st.data_ptr() if stats and n else (0x1000 if stats else None),
                                                torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return (x.cpu().numpy() if frames else None), (frontend.stats64_tensor_to_numpy(st) if stats else None)


def _assert_stats(got, want):
    assert got.shape == want.shape and got.dtype == R.STATS64_DTYPE
    for k in R.STATS64_DTYPE.names:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def _check_frames(x, iq, fmt, n, hop, level, remove_dc):
    x64 = R.frames(iq, fmt, level, hop, remove_dc, n)
    assert np.isfinite(x).all()
    err = np.abs(x.astype(np.float64) - x64)
    worst = float((err / np.where(x64 != 0, np.abs(x64), 1.0)).max()) if n else 0.0
    print(f"{fmt} hop {hop} n {n} level {level} dc {remove_dc}: largest relative error {worst / 2.0 ** -24:.3f} x 2^-24")
    assert (err <= REL * np.abs(x64)).all(), worst
    zero = (R.centred(iq, fmt, hop, remove_dc, n) == 0) | (R.stats(iq, fmt, hop, remove_dc, n)["energy"] == 0)[:, None, None]
    assert (x[zero] == 0).all()


# ---------------------------------------------------------------------------------------------------------------- 1. statistics
@pytest.mark.parametrize("n", [0, 1, 2, 7, 9, 255, 4097])
@pytest.mark.parametrize("hop", [128, 64, 1, 37])
@pytest.mark.parametrize("fmt", ["ci8", "ci16"])
def test_stats_are_exact_and_the_three_runs_agree(fmt, hop, n):
    buf = _capture(fmt, n, hop, seed=1000 * hop + n)
    iq = buf[2:]
    dev = torch.from_numpy(buf).cuda()[2:]
    pair = R.PAIR_BYTES[fmt]
    assert n == 0 or dev.data_ptr() % (2 * pair) == pair          # one pair into the allocation: aligned to a pair, no better
    want = R.stats_records(iq, fmt, hop, True, n)
    _, only = _run(dev, fmt, n, hop, 7.8e-3, DC, False, True)
    x, both = _run(dev, fmt, n, hop, 7.8e-3, DC, True, True)
    _assert_stats(only, want)
    _assert_stats(both, want)
    x_alone, _ = _run(dev, fmt, n, hop, 7.8e-3, DC, True, False)
    np.testing.assert_array_equal(x_alone.view(np.uint32), x.view(np.uint32))
    _check_frames(x, iq, fmt, n, hop, 7.8e-3, True)
    _, nodc = _run(dev, fmt, n, hop, 7.8e-3, 0, False, True)
    _assert_stats(nodc, R.stats_records(iq, fmt, hop, False, n))
    W = -(-128 // hop)
    if n > 6 * W:      # windows 0, W, ..., 6W are the special segments themselves
        _, bq, be = R.BOUNDS[fmt]
        assert both["sum_sq"][0] == bq and both["energy"][0] == 0 and nodc["energy"][0] == be          # all minimum
        assert both["energy"][W] == 0 and both["energy"][3 * W] == 0 and both["energy"][4 * W] == 0 and both["sum_sq"][4 * W] == 0
        assert both["energy"][2 * W] == both["energy"].max() > (be >> 1)                               # alternating: the largest E
        assert not x[0].any() and not x[W].any() and not x[3 * W].any() and not x[4 * W].any()
        assert both["energy"][5 * W] > 0 and both["energy"][6 * W] > 0 and x[6 * W].any()


@pytest.mark.parametrize("fmt", ["ci8", "ci16"])
def test_stats_past_the_grid_cap(fmt):
    """n just beyond grid cap x windows per work-group at hop 1: the stride loop runs, on a capture of 128 K pairs."""
    n, hop = GRID_CAP_WINDOWS + 11, 1
    buf = _capture(fmt, n, hop, seed=3)
    dev = torch.from_numpy(buf).cuda()[2:]
    _, got = _run(dev, fmt, n, hop, 1.0, DC, False, True)
    _assert_stats(got, R.stats_records(buf[2:], fmt, hop, True, n))


# ---------------------------------------------------------------------------------------------------------------- 2. frames
@pytest.mark.parametrize("level", [7.8e-3, 1.0, 3.0e4])
@pytest.mark.parametrize("remove_dc", [True, False])
@pytest.mark.parametrize("fmt", ["ci8", "ci16"])
def test_frames_within_the_derived_bound(fmt, remove_dc, level):
    for hop, n in ((128, 600), (37, 2049)):
        buf = _capture(fmt, n, hop, seed=77)
        # a quiet stretch too (a few LSB): E far below 2^24, the other end of the conversion
        buf[2 + 2 * hop * 300: 2 + 2 * hop * 300 + 4096] = np.random.default_rng(5).integers(-3, 4, size=4096)
        dev = torch.from_numpy(buf).cuda()[2:]
        x, st = _run(dev, fmt, n, hop, level, DC if remove_dc else 0, True, True)
        _assert_stats(st, R.stats_records(buf[2:], fmt, hop, remove_dc, n))
        _check_frames(x, buf[2:], fmt, n, hop, level, remove_dc)


# ---------------------------------------------------------------------------------------------------------------- 3. identities
def _run_u8(dev, n, hop, level, flags):
    x = torch.full((n, 2, 128), float("nan"), dtype=torch.float32, device="cuda")
    st = torch.full((n, 4), -1, dtype=torch.int32, device="cuda")
    _cabi.check(_cabi.lib().mdc_iq_u8_windows_norm(dev.data_ptr(), n, hop, level, flags, x.data_ptr(), st.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return x.cpu().numpy(), frontend.stats_tensor_to_numpy(st)


@pytest.mark.parametrize("hop", [128, 37])
def test_u8_bytes_with_flipped_sign_bits_read_as_ci8(hop):
    n = 3001
    u8 = np.random.default_rng(hop).integers(0, 256, size=2 * (hop * (n - 1) + 128), dtype=np.uint8)
    u8[:256], u8[2 * hop * 4: 2 * hop * 4 + 256] = 0, 255
    i8 = (u8 ^ 0x80).view(np.int8)
    for level in (7.8e-3, 3.0e4):
        xu, su = _run_u8(torch.from_numpy(u8).cuda(), n, hop, level, DC)
        xi, si = _run(torch.from_numpy(i8).cuda(), "ci8", n, hop, level, DC, True, True)
        np.testing.assert_array_equal(xi.view(np.uint32), xu.view(np.uint32))           # s_u8 = 2 s_i8 + 1: a DC offset and a factor 2
        np.testing.assert_array_equal(4 * si["energy"], su["energy"].astype(np.uint64))


@pytest.mark.parametrize("hop", [128, 37])
def test_ci8_widened_to_ci16(hop):
    n = 3001
    buf = _capture("ci8", n, hop, seed=21)[2:]
    wide = (buf.astype(np.int16) * 256).astype("<i2")
    for flags in (DC, 0):
        x8, s8 = _run(torch.from_numpy(buf).cuda(), "ci8", n, hop, 7.8e-3, flags, True, True)
        x16, s16 = _run(torch.from_numpy(wide).cuda(), "ci16", n, hop, 7.8e-3, flags, True, True)
        np.testing.assert_array_equal(x16.view(np.uint32), x8.view(np.uint32))
        np.testing.assert_array_equal(s16["sum_i"], 256 * s8["sum_i"])
        np.testing.assert_array_equal(s16["sum_q"], 256 * s8["sum_q"])
        np.testing.assert_array_equal(s16["sum_sq"], 65536 * s8["sum_sq"])
        np.testing.assert_array_equal(s16["energy"], 65536 * s8["energy"])


@pytest.mark.parametrize("hop", [128, 16, 37])
def test_cu8_through_the_new_entries_is_the_old_ones(hop):
    n = 3001
    u8 = np.random.default_rng(hop + 1).integers(0, 256, size=2 * (hop * (n - 1) + 128) + 2, dtype=np.uint8)
    u8[2:258] = 7
    dev = torch.from_numpy(u8).cuda()[2:]
    for flags in (DC, 0):
        xo, so = _run_u8(dev, n, hop, 0.5, flags)
        xn, sn = _run(dev, "cu8", n, hop, 0.5, flags, True, True)
        np.testing.assert_array_equal(xn.view(np.uint32), xo.view(np.uint32))
        _, only = _run(dev, "cu8", n, hop, 0.5, flags, False, True)
        for got in (sn, only):
            for k in R.STATS64_DTYPE.names:
                np.testing.assert_array_equal(got[k].astype(np.int64), so[k].astype(np.int64), err_msg=k)
        x_alone, _ = _run(dev, "cu8", n, hop, 0.5, flags, True, False)
        np.testing.assert_array_equal(x_alone.view(np.uint32), xo.view(np.uint32))
    old = frontend.frames_from_iq_u8(dev, 0.013, hop=hop)
    new = frontend.frames_from_iq(dev, "cu8", 0.013, hop=hop)
    assert torch.equal(old, new)
    _assert_stats(frontend.window_stats_iq(dev, "cu8", hop=hop), R.stats_records(u8[2:], "cu8", hop, True, n))


@pytest.mark.parametrize("fmt", ["ci8", "ci16"])
@pytest.mark.parametrize("hop", [128, 37])
def test_dc_offset_changes_nothing_under_remove_dc(fmt, hop):
    n = 3001
    amp = R.AMPLITUDE[fmt] // 2
    iq = np.random.default_rng(hop).integers(-amp, amp, size=2 * (hop * (n - 1) + 128)).astype(R.DTYPE[fmt])
    oi, oq = (23, -31) if fmt == "ci8" else (9001, -12345)
    shifted = iq.reshape(-1, 2).copy()
    shifted[:, 0] += oi
    shifted[:, 1] += oq
    shifted = shifted.reshape(-1)
    xa, sa = _run(torch.from_numpy(iq).cuda(), fmt, n, hop, 7.8e-3, DC, True, True)
    xb, sb = _run(torch.from_numpy(shifted).cuda(), fmt, n, hop, 7.8e-3, DC, True, True)
    np.testing.assert_array_equal(xa.view(np.uint32), xb.view(np.uint32))
    np.testing.assert_array_equal(sa["energy"], sb["energy"])
    np.testing.assert_array_equal(sb["sum_i"] - sa["sum_i"], 128 * oi)
    np.testing.assert_array_equal(sb["sum_q"] - sa["sum_q"], 128 * oq)
    assert not np.array_equal(sa["sum_sq"], sb["sum_sq"])


# ---------------------------------------------------------------------------------------------------------------- 4. plain conversion
@pytest.mark.parametrize("hop", [128, 37])
@pytest.mark.parametrize("fmt", ["ci8", "ci16"])
def test_plain_conversion_is_the_f32_product(fmt, hop):
    n = 1027
    buf = _capture(fmt, n, hop, seed=8)
    dev = torch.from_numpy(buf).cuda()[2:]
    for scale in (None, 0.02 / 3.0):
        x = frontend.frames_from_iq(dev, fmt, scale, hop=hop)
        torch.cuda.synchronize()
        want = R.plain_frames(buf[2:], fmt, (1.0 / R.AMPLITUDE[fmt]) if scale is None else scale, hop, n)
        np.testing.assert_array_equal(x.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert frontend.frames_from_iq(dev[:254], fmt, hop=1).shape == (0, 2, 128)


def test_frontend_functions_and_power():
    hop, n = 16, 3000
    buf = _capture("ci16", n, hop, seed=9)[2:]
    st = frontend.window_stats_iq(buf, "ci16_le", hop=hop)
    want = R.stats_records(buf, "ci16", hop, True, n)
    assert st.dtype == _cabi.IQ_WINDOW_STATS64
    _assert_stats(st, want)
    np.testing.assert_array_equal(frontend.window_power_dbfs(st, "ci16"), R.power_dbfs(want["energy"], "ci16"))
    x, st_dev = frontend.normalized_frames_from_iq(buf.reshape(-1, 2), "ci16", level=0.5, hop=hop, return_stats=True)
    assert x.shape == (n, 2, 128) and x.is_cuda
    _assert_stats(frontend.stats64_tensor_to_numpy(st_dev), want)
    np.testing.assert_array_equal(frontend.window_power_dbfs(st_dev, "ci16"), R.power_dbfs(want["energy"], "ci16"))
    rms = torch.sqrt((x.double() ** 2).sum(dim=(1, 2)) / 128).cpu().numpy()
    live = want["energy"] > 0
    assert np.abs(rms[live] / 0.5 - 1).max() < 1e-6 and not rms[~live].any()
    be = frontend.normalized_frames_from_iq(buf.astype(">i2"), "ci16", level=0.5, hop=hop)          # big-endian numpy: converted
    assert torch.equal(be, x)


# ---------------------------------------------------------------------------------------------------------------- 5. composition
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


_varied = {}


def _varied_capture(fmt, n, hop, seed):
    """Level-varied samples: blocks of 2,048 pairs with amplitudes from 2 LSB to a third of full scale around a drifting DC
    offset, so that window powers spread over tens of dB.  Computed once per (fmt, n, hop, seed)."""
    key = (fmt, n, hop, seed)
    if key not in _varied:
        rng = np.random.default_rng(seed)
        ns = 2 * (hop * (n - 1) + 128)
        full = R.AMPLITUDE[fmt]
        amps = [2, 5, 11, full // 400 + 20, full // 60, full // 9, full // 3]
        amp = np.repeat(rng.choice(amps, size=ns // 4096 + 1), 4096)[:ns]
        mid = np.repeat(rng.integers(-full // 50 - 3, full // 50 + 4, size=ns // 4096 + 1), 4096)[:ns]
        v = np.clip(np.rint(mid + amp * rng.standard_normal(ns) / 3), R.SAMPLE_MIN[fmt], R.SAMPLE_MAX[fmt]).astype(R.DTYPE[fmt])
        st = R.stats(v, fmt, hop, True, n)
        _varied[key] = (v, R.stats_records(v, fmt, hop, True, n), R.power_dbfs(st["energy"], fmt))
    return _varied[key]


@pytest.mark.parametrize("hop", [128, 16])
@pytest.mark.parametrize("name,dtype", NETS)
def test_normalised_predict_equals_the_two_calls_and_the_host_driver(name, dtype, hop):
    n, fmt = 2500, "ci16"
    m = _net(name, dtype)
    Cn = m.topology.classes
    iq, want_st, power_ref = _varied_capture(fmt, n, hop, seed=31 + hop)
    dev = torch.from_numpy(iq).cuda()
    level = 7.8e-3
    # by hand: mdc_iq_windows_norm, then forward_device
    x, st = frontend.normalized_frames_from_iq(dev, fmt, level=level, hop=hop, return_stats=True)
    p_hand, l_hand, _ = m.forward_device(x)
    _assert_stats(frontend.stats64_tensor_to_numpy(st), want_st)
    thr = float(np.median(power_ref))
    squelched = power_ref < thr
    assert 0 < squelched.sum() < n
    for bs in (0, 700):      # device tensor in: whole and chunked
        p, l, pw = m.predict_iq(dev, fmt, hop=hop, normalize="rms", level=level, batch_size=bs, return_power=True)
        assert torch.equal(p, p_hand) and torch.equal(l, l_hand), (name, dtype, hop, bs)
        np.testing.assert_allclose(pw.cpu().numpy(), power_ref, rtol=0, atol=1e-9)
    p, l = m.predict_iq(dev.view(-1, 2), "ci16_le", hop=hop, normalize="rms", level=level, squelch_dbfs=thr)
    assert torch.equal(p, p_hand)
    np.testing.assert_array_equal(l.cpu().numpy(), np.where(squelched, -1, l_hand.cpu().numpy()))
    # numpy in: the host driver, through the mirror ...
    p, l, pw = m.predict_iq(iq, fmt, hop=hop, normalize="rms", level=level, squelch_dbfs=thr, return_power=True)
    np.testing.assert_array_equal(p.view(np.uint32), p_hand.cpu().numpy().view(np.uint32))
    np.testing.assert_array_equal(l, np.where(squelched, -1, l_hand.cpu().numpy()))
    np.testing.assert_array_equal(pw, power_ref)
    # ... and straight through the ABI at chunk sizes {default, 1,000, n}, with and without the statistics
    L, h = m._lib(), m._engine()
    for chunk in (0, 1000, n):
        for with_stats in (True, False):
            probs, labels = np.full((n, Cn), np.nan, np.float32), np.full((n,), -7, np.int32)
            stats = np.zeros((n,), _cabi.IQ_WINDOW_STATS64)
            m._check(L.mdc_predict_host_iq_norm(h, iq.ctypes.data, FMT[fmt], n, hop, level, DC, probs.ctypes.data, labels.ctypes.data,
                                                stats.ctypes.data if with_stats else None, chunk))
            np.testing.assert_array_equal(probs.view(np.uint32), p_hand.cpu().numpy().view(np.uint32), err_msg=str(chunk))
            np.testing.assert_array_equal(labels, l_hand.cpu().numpy())
            if with_stats:
                _assert_stats(stats, want_st)


@pytest.mark.parametrize("name,dtype", NETS)
def test_normalize_none_is_windows_plus_forward_and_cu8_is_predict_iq_u8(name, dtype):
    n, hop = 1500, 16
    m = _net(name, dtype)
    for fmt in ("ci16", "ci8"):
        iq = _varied_capture(fmt, n, hop, seed=5)[0]
        dev = torch.from_numpy(iq).cuda()
        scale = 0.02 / R.AMPLITUDE[fmt]
        p_ref, l_ref, _ = m.forward_device(frontend.frames_from_iq(dev, fmt, scale, hop=hop))
        for bs in (0, 400):
            p, l = m.predict_iq(dev, fmt, scale, hop=hop, batch_size=bs)
            assert torch.equal(p, p_ref) and torch.equal(l, l_ref), (fmt, bs)
        for bs in (0, 400):
            p_np, l_np = m.predict_iq(iq, fmt, scale, hop=hop, batch_size=bs)
            np.testing.assert_array_equal(p_np.view(np.uint32), p_ref.cpu().numpy().view(np.uint32))
            np.testing.assert_array_equal(l_np, l_ref.cpu().numpy())
    u8 = (_varied_capture("ci8", n, hop, seed=5)[0].view(np.uint8) ^ 0x80)
    dev = torch.from_numpy(u8).cuda()
    for src in (dev, u8):
        for kw in ({"scale": 0.02 / 127.5}, {"normalize": "rms", "squelch_dbfs": -30.0, "return_power": True}, {"normalize": "rms", "remove_dc": False}):
            a, b = m.predict_iq(src, "cu8", hop=hop, **kw), m.predict_iq_u8(src, hop=hop, **kw)
            assert len(a) == len(b)
            for u, v in zip(a, b):
                if isinstance(u, torch.Tensor):
                    assert u.dtype == v.dtype and torch.equal(u, v)
                else:
                    assert u.dtype == v.dtype
                    np.testing.assert_array_equal(u, v)
    # MDC_IQ_CU8 straight through the new host drivers: the frames path serves cnn.py's net too
    L, h, Cn = m._lib(), m._engine(), m.topology.classes
    p_old, l_old = m.predict_iq_u8(dev, 0.02 / 127.5, hop=hop)
    probs, labels = np.full((n, Cn), np.nan, np.float32), np.full((n,), -7, np.int32)
    m._check(L.mdc_predict_host_iq(h, u8.ctypes.data, _cabi.IQ_CU8, n, hop, 0.02 / 127.5, probs.ctypes.data, labels.ctypes.data, 600))
    np.testing.assert_array_equal(probs.view(np.uint32), p_old.cpu().numpy().view(np.uint32))
    np.testing.assert_array_equal(labels, l_old.cpu().numpy())
    p_old, l_old, pw_old = m.predict_iq_u8(dev, hop=hop, normalize="rms", return_power=True)
    stats = np.zeros((n,), _cabi.IQ_WINDOW_STATS64)
    m._check(L.mdc_predict_host_iq_norm(h, u8.ctypes.data, _cabi.IQ_CU8, n, hop, 7.8e-3, DC, probs.ctypes.data, labels.ctypes.data, stats.ctypes.data, 600))
    np.testing.assert_array_equal(probs.view(np.uint32), p_old.cpu().numpy().view(np.uint32))
    np.testing.assert_array_equal(labels, l_old.cpu().numpy())
    np.testing.assert_allclose(frontend.window_power_dbfs(stats, "cu8"), pw_old.cpu().numpy(), rtol=0, atol=1e-9)


def test_host_drivers_refuse_null_and_device_input_and_accept_nothing():
    m = _net("dep3", "f32")
    L, h = m._lib(), m._engine()
    dev = torch.zeros(4096, dtype=torch.int16, device="cuda")
    out = np.empty((16, 3), np.float32)
    for fmt in FMT.values():
        assert L.mdc_predict_host_iq(h, None, fmt, 2, 128, 1.0, out.ctypes.data, None, 0) == -22 and b"null input" in L.mdc_last_error()
        assert L.mdc_predict_host_iq_norm(h, None, fmt, 2, 128, 1.0, DC, out.ctypes.data, None, None, 0) == -22 and b"null input" in L.mdc_last_error()
        assert L.mdc_predict_host_iq(h, None, fmt, 0, 128, 1.0, None, None, 0) == 0
        assert L.mdc_predict_host_iq_norm(h, None, fmt, 0, 128, 1.0, DC, None, None, None, 0) == 0
        assert L.mdc_predict_host_iq_norm(h, dev.data_ptr(), fmt, 4, 128, 1.0, DC, out.ctypes.data, None, None, 0) == -22
        assert b"device memory" in L.mdc_last_error()
    p, l = m.predict_iq(np.zeros(4096, np.int16), "ci16", normalize="rms")          # constant windows: zero frames, finite rows
    assert np.isfinite(p).all() and p.shape == (16, 3)
    p, l = m.predict_iq(np.zeros(100, np.int8), "ci8", hop=3)                      # shorter than a window
    assert p.shape == (0, 3) and l.shape == (0,)
    m._release()


# ---------------------------------------------------------------------------------------------------------------- 6. graph capture
def test_norm_and_forward_are_capturable():
    n, hop, fmt = 600, 16, "ci16"
    m = _net("vtcnn2", "bf16")
    dev = torch.from_numpy(_varied_capture(fmt, n, hop, seed=1)[0]).cuda()
    m.predict_iq(dev, fmt, hop=hop, normalize="rms", return_power=True)                  # warm: workspace, code objects
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        p1, l1, w1 = m.predict_iq(dev, fmt, hop=hop, normalize="rms", return_power=True)
    for seed in (2, 3):
        dev.copy_(torch.from_numpy(_varied_capture(fmt, n, hop, seed=seed)[0]).cuda())      # same buffer, new capture
        p1.zero_()
        l1.fill_(-5)
        g.replay()
        torch.cuda.synchronize()
        pe, le, we = m.predict_iq(dev, fmt, hop=hop, normalize="rms", return_power=True)
        torch.cuda.synchronize()
        assert torch.equal(p1, pe) and torch.equal(l1, le) and torch.equal(w1, we), seed


# ---------------------------------------------------------------------------------------------------------------- 7. trained net
QUANTISED = [("ci16", 50), ("ci16", 30000), ("ci8", 100)]      # format, largest |sample| of the quantised batch in LSB
DC_LSB = (3, -2)


def _trained_record():
    """Computed once per process, by the f64 oracle only: the held-out frames quantised per QUANTISED (+ DC), normalised by
    the reference, and the oracle's labels on them."""
    import trained_vtcnn2 as T
    from oracle import oracle_np as O
    if "iq_formats" not in T._cache:
        w, _ = T.trained()
        x, _, _, _ = T.held_out()
        rec = {"weights": w, "q": {}}
        for fmt, peak in QUANTISED:
            iq = R.quantise_frames(x, fmt, peak, DC_LSB)
            xn = R.frames(iq, fmt, 7.8e-3, 128, True)
            rec["q"][(fmt, peak)] = {"iq": iq, "oracle_labels": O.forward("vtcnn2", xn, w, dtype=np.float64)["labels"]}
        T._cache["iq_formats"] = rec
    return T._cache["iq_formats"]


def _floors():
    from test_label_agreement_gpu import MODES
    return MODES + [("f32", 0.9995)]


@pytest.mark.parametrize("mode", ["f32", "bf16", "fp8", "fp8+bf16feat"])
@pytest.mark.parametrize("fmt,peak", QUANTISED)
def test_trained_net_labels_against_the_oracle_on_the_normalised_frames(fmt, peak, mode):
    """The floors are test_label_agreement_gpu.MODES' (+ f32 at 0.9995), imported, not restated."""
    floor = dict(_floors())[mode]
    rec = _trained_record()
    q = rec["q"][(fmt, peak)]
    m = VTCNN2(Topology.vtcnn2(11), dtype="fp8" if mode.startswith("fp8") else mode, fp8_bf16_features=mode == "fp8+bf16feat")
    m.set_weights(rec["weights"])
    lab_dev = m.predict_iq(torch.from_numpy(q["iq"]).cuda(), fmt, normalize="rms")[1].cpu().numpy()
    lab_host = m.predict_iq(q["iq"], fmt, normalize="rms")[1]
    np.testing.assert_array_equal(lab_dev, lab_host)
    agree = float((lab_dev == q["oracle_labels"]).mean())
    print(f"{fmt} peak {peak} LSB, {mode}: {agree:.5f} of labels equal the f64 oracle's on the normalised frames (floor {floor})")
    assert agree >= floor, agree
