"""Signed 8- and 16-bit I/Q captures (include/mdc.h: mdc_iq_windows, mdc_iq_windows_norm, mdc_predict_host_iq,
mdc_predict_host_iq_norm) without a GPU: the four entry points validate their arguments before any device call, the binding
describes the 64-bit record, the squelch threshold is the dBFS comparison per format, and the numpy restatement the GPU tests
hold the kernels to (tests/iq_formats_ref.py) has the properties the header states -- the identities
tests/test_iq_formats_gpu.py then demands of the kernels."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import iq_formats_ref as R
import iq_norm_ref as R8
from modulationdetectioncnn_amd import _cabi, frontend

CU8, CI8, CI16 = _cabi.IQ_CU8, _cabi.IQ_CI8, _cabi.IQ_CI16
DC = _cabi.IQ_REMOVE_DC


def _lib():
    L = _cabi.lib()
    L.mdc_last_error.restype = ctypes.c_char_p
    return L


def test_device_entry_points_validate_their_arguments_without_gpu():
    L = _lib()
    buf = (ctypes.c_uint8 * 2048)()
    out = (ctypes.c_uint8 * 8192)()
    iq = (ctypes.addressof(buf) + 15) & ~15
    x = (ctypes.addressof(out) + 15) & ~15
    w, f = L.mdc_iq_windows, L.mdc_iq_windows_norm
    for fmt in (-1, 3, 99):
        assert w(iq, fmt, 2, 128, 1.0, x, None) == -22 and b"format" in L.mdc_last_error()
        assert f(iq, fmt, 2, 128, 1.0, DC, x, None, None) == -22 and b"format" in L.mdc_last_error()
    for fmt in (CU8, CI8, CI16):
        assert w(iq, fmt, -1, 128, 1.0, x, None) == -22 and b"negative" in L.mdc_last_error()
        assert f(iq, fmt, -1, 128, 1.0, DC, x, None, None) == -22 and b"negative" in L.mdc_last_error()
        for hop in (0, -3, (1 << 24) + 1):
            assert w(iq, fmt, 2, hop, 1.0, x, None) == -22 and b"hop" in L.mdc_last_error()
            assert f(iq, fmt, 2, hop, 1.0, DC, x, None, None) == -22 and b"hop" in L.mdc_last_error()
        off = 2 if fmt == CI16 else 1                          # one byte off a pair (8-bit), two bytes off (16-bit)
        assert w(iq + off, fmt, 2, 16, 1.0, x, None) == -22 and b"pair" in L.mdc_last_error()
        assert f(iq + off, fmt, 2, 16, 1.0, DC, x, None, None) == -22 and b"pair" in L.mdc_last_error()
        assert f(iq + off, fmt, 2, 16, 1.0, DC, None, x, None) == -22 and b"pair" in L.mdc_last_error()
        assert w(None, fmt, 2, 16, 1.0, x, None) == -22 and b"null buffer" in L.mdc_last_error()
        assert w(iq, fmt, 2, 16, 1.0, None, None) == -22 and b"null buffer" in L.mdc_last_error()
        assert f(None, fmt, 2, 16, 1.0, DC, x, None, None) == -22 and b"null buffer" in L.mdc_last_error()
        assert f(iq, fmt, 2, 16, 1.0, DC, None, None, None) == -22 and b"null buffer" in L.mdc_last_error()      # both outputs NULL
        for level in (0.0, -1.0, float("nan"), float("inf")):
            assert f(iq, fmt, 2, 128, level, DC, x, None, None) == -22 and b"level" in L.mdc_last_error(), level
        assert f(iq, fmt, 2, 128, 1.0, 2, x, None, None) == -22 and b"flag" in L.mdc_last_error()
        assert f(iq, fmt, 2, 16, 1.0, DC, x + 4, None, None) == -22 and b"8-byte" in L.mdc_last_error()
        assert f(iq, fmt, 2, 16, 1.0, DC, None, x + 8, None) == -22 and b"16-byte" in L.mdc_last_error()
        assert w(iq, fmt, 2, 16, 1.0, x + 4, None) == -22 and b"8-byte" in L.mdc_last_error()
        # n = 0: nothing to launch, whatever the buffers
        assert w(None, fmt, 0, 16, 1.0, None, None) == 0
        assert f(None, fmt, 0, 16, 1.0, 0, None, None, None) == 0
    # the message names the pair size
    assert w(iq + 2, CI16, 2, 16, 1.0, x, None) == -22 and b"4-byte" in L.mdc_last_error()
    assert w(iq + 1, CI8, 2, 16, 1.0, x, None) == -22 and b"2-byte" in L.mdc_last_error()


def test_host_drivers_validate_their_arguments_without_gpu():
    L = _lib()
    buf = (ctypes.c_uint8 * 2048)()
    iq = ctypes.addressof(buf)
    h, hn = L.mdc_predict_host_iq, L.mdc_predict_host_iq_norm
    for fmt in (CU8, CI8, CI16):
        assert h(None, iq, fmt, 2, 128, 1.0, None, None, 0) == -22 and b"null model" in L.mdc_last_error()
        assert hn(None, iq, fmt, 2, 128, 1.0, DC, None, None, None, 0) == -22 and b"null model" in L.mdc_last_error()
        assert h(None, iq, fmt, 0, 128, 1.0, None, None, 0) == -22 and b"null model" in L.mdc_last_error()
        assert hn(None, iq, fmt, 2, 0, 1.0, DC, None, None, None, 0) == -22 and b"hop" in L.mdc_last_error()
        assert hn(None, iq, fmt, 2, 128, 0.0, DC, None, None, None, 0) == -22 and b"level" in L.mdc_last_error()
        assert hn(None, iq, fmt, 2, 128, float("nan"), DC, None, None, None, 0) == -22 and b"level" in L.mdc_last_error()
        assert hn(None, iq, fmt, 2, 128, 1.0, 8, None, None, None, 0) == -22 and b"flag" in L.mdc_last_error()
    for fmt in (CI8, CI16):
        assert h(None, iq, fmt, 2, 0, 1.0, None, None, 0) == -22 and b"hop" in L.mdc_last_error()
    for fmt in (-1, 3):
        assert h(None, iq, fmt, 2, 128, 1.0, None, None, 0) == -22 and b"format" in L.mdc_last_error()
        assert hn(None, iq, fmt, 2, 128, 1.0, DC, None, None, None, 0) == -22 and b"format" in L.mdc_last_error()


def test_binding_describes_the_formats_and_the_64_bit_record():
    assert _cabi.IQ_WINDOW_STATS64.itemsize == 32 and _cabi.IQ_WINDOW_STATS64 == R.STATS64_DTYPE
    assert {"mdc_iq_windows", "mdc_iq_windows_norm", "mdc_predict_host_iq", "mdc_predict_host_iq_norm"} <= set(_cabi.EXPORTS)
    assert (_cabi.IQ_CU8, _cabi.IQ_CI8, _cabi.IQ_CI16) == (0, 1, 2) == tuple(R.FORMATS[k] for k in ("cu8", "ci8", "ci16"))
    assert _cabi.ABI_VERSION == 5 and _cabi.IQ_WINDOW_STATS.itemsize == 16
    for name, fmt in R.FORMATS.items():
        assert _cabi.IQ_PAIR_BYTES[fmt] == R.PAIR_BYTES[name] and _cabi.IQ_SAMPLE_DTYPE[fmt] == R.DTYPE[name]
        assert frontend.sample_format_id(name) == fmt and frontend.full_scale_energy(name) == R.full_scale_energy(name)
    assert frontend.sample_format_id("ci16_le") == CI16 and frontend.sample_format_id("CI8") == CI8
    with pytest.raises(ValueError):
        frontend.sample_format_id("cf32")


def test_window_count_takes_the_pair_size():
    assert frontend.window_count(512) == 2 == frontend.window_count(1024, pair_bytes=4)
    assert frontend.window_count(4 * (128 + 37 * 9), 37, 4) == 10 == frontend.window_count(2 * (128 + 37 * 9), 37)
    assert frontend.window_count(4 * 127, 1, 4) == 0
    with pytest.raises(ValueError):
        frontend.window_count(768, 128, 4)                      # one and a half 16-bit frames
    with pytest.raises(ValueError):
        frontend.window_count(1026, 16, 4)                      # half a pair


def test_host_samples_checks_the_dtype_and_converts_byte_order_only():
    be = np.arange(-300, 212, dtype=">i2")
    le = frontend.host_samples(be.reshape(-1, 2), CI16)
    assert le.dtype == np.dtype("<i2") and le.ndim == 1 and np.array_equal(le.astype(np.int64), np.arange(-300, 212))
    assert frontend.host_samples(np.zeros((4, 2), np.int8), CI8).shape == (8,)
    for bad, fmt in ((np.zeros(4, np.uint8), CI8), (np.zeros(4, np.int8), CU8), (np.zeros(4, np.int32), CI16), (np.zeros(4, np.uint16), CI16),
                     (np.zeros(4, np.float32), CI16), ([1, 2, 3, 4], CI8)):
        with pytest.raises(TypeError):
            frontend.host_samples(bad, fmt)


@pytest.mark.parametrize("fmt", ["cu8", "ci8", "ci16"])
def test_squelch_threshold_is_the_dbfs_comparison(fmt):
    top = 128 * 256 * max(abs(R.SAMPLE_MIN[fmt] * 2 - 255 if fmt == "cu8" else R.SAMPLE_MIN[fmt]), 1) ** 2      # the largest E of the format
    assert top == R.BOUNDS[fmt][2]
    full = R.full_scale_energy(fmt)
    rng = np.random.default_rng(6)
    energies = np.unique(np.concatenate([[0, 1, 2, full - 1, full, full + 1, top - 1, top], rng.integers(0, top + 1, size=3000),
                                         np.rint(full * 10.0 ** (rng.uniform(-90, 3.02, size=3000) / 10)).astype(np.int64)]))
    assert R.power_dbfs([top], fmt)[0] < 3.011 and R.power_dbfs([full], fmt)[0] == 0.0      # +3 dB at the very most
    for sq in (-90.0, -60.0, -30.0, -12.5, -1e-9, 0.0, 2.9, 3.0, 3.02, 10.0, float("-inf"), float("inf")):
        thr = frontend.squelch_energy_threshold(sq, fmt)
        np.testing.assert_array_equal(energies < thr, R.power_dbfs(energies, fmt) < sq, err_msg=str(sq))
        if fmt == "cu8":
            assert thr == frontend.squelch_energy_threshold(sq)          # one argument: what it returned before
    rec = np.zeros(energies.size, _cabi.IQ_WINDOW_STATS64)
    rec["energy"] = energies
    np.testing.assert_array_equal(frontend.window_power_dbfs(rec, fmt), R.power_dbfs(energies, fmt))
    cols = np.zeros((energies.size, 4), np.int64)
    cols[:, 3] = energies
    np.testing.assert_array_equal(frontend.window_power_dbfs(cols, fmt), R.power_dbfs(energies, fmt))


def test_squelch_threshold_of_cu8_is_unchanged():
    for sq, want in ((-30.0, 1065370), (0.0, R8.FULL_SCALE_ENERGY), (10.0, 1 << 31), (float("-inf"), 0)):
        assert frontend.squelch_energy_threshold(sq) == want == frontend.squelch_energy_threshold(sq, "cu8")


def test_predict_iq_refuses_wrong_dtypes_and_contradicting_arguments():
    from modulationdetectioncnn_amd import VTCNN2
    m = VTCNN2.synthetic("deployed3")
    with pytest.raises(TypeError):
        m.predict_iq(np.zeros(512, np.uint8), "ci8")
    with pytest.raises(TypeError):
        m.predict_iq(np.zeros(512, np.int8), "ci16")
    with pytest.raises(TypeError):
        m.predict_iq(np.zeros(512, np.int16), "cu8")
    with pytest.raises(ValueError):
        m.predict_iq(np.zeros(512, np.int16), "cf32")
    iq = np.zeros(512, np.int16)
    with pytest.raises(ValueError, match="scale"):
        m.predict_iq(iq, "ci16", scale=0.01, normalize="rms")
    with pytest.raises(ValueError, match="normalize"):
        m.predict_iq(iq, "ci16", normalize="peak")
    with pytest.raises(ValueError, match="normalize='rms'"):
        m.predict_iq(iq, "ci16", squelch_dbfs=-30.0)
    with pytest.raises(ValueError, match="normalize='rms'"):
        m.predict_iq(iq, "ci16", return_power=True)
    with pytest.raises(ValueError, match="level"):
        m.predict_iq(iq, "ci16", normalize="rms", level=0.0)


# ---------------------------------------------------------------------------------------------------------------- the reference
def _capture(fmt, seed, nsamples, lo=None, hi=None):
    lo = R.SAMPLE_MIN[fmt] if lo is None else lo
    hi = R.SAMPLE_MAX[fmt] + 1 if hi is None else hi
    return np.random.default_rng(seed).integers(lo, hi, size=nsamples).astype(R.DTYPE[fmt])


def _extremes(fmt):
    """windows of 256 samples: all minimum, all maximum, alternating minimum / maximum, I minimum with Q maximum, all zero"""
    lo, hi, dt = R.SAMPLE_MIN[fmt], R.SAMPLE_MAX[fmt], R.DTYPE[fmt]
    alt = np.empty(256, dt)
    alt[0::4], alt[1::4], alt[2::4], alt[3::4] = lo, lo, hi, hi
    return np.concatenate([np.full(256, lo, dt), np.full(256, hi, dt), alt, np.tile(np.array([lo, hi], dt), 128), np.zeros(256, dt)])


def test_reference_of_cu8_is_the_existing_reference():
    iq = _capture("cu8", 1, 2 * (128 + 37 * 40))
    for dc in (True, False):
        a, b = R.stats(iq, "cu8", 37, dc), R8.stats(iq, 37, dc)
        for k in a:
            np.testing.assert_array_equal(a[k], b[k])
        np.testing.assert_array_equal(R.frames(iq, "cu8", 0.3, 37, dc), R8.frames(iq, 0.3, 37, dc))
    np.testing.assert_array_equal(R.power_dbfs(a["energy"], "cu8"), R8.power_dbfs(a["energy"]))


@pytest.mark.parametrize("fmt", ["ci8", "ci16"])
@pytest.mark.parametrize("remove_dc", [True, False])
def test_reference_energy_is_the_exact_centred_sum_within_the_headers_bounds(fmt, remove_dc):
    iq = np.concatenate([_extremes(fmt), _capture(fmt, 4, 2 * (128 + 37 * 11))])
    st = R.stats(iq, fmt, 37, remove_dc)
    s = R.windows(iq, fmt, 37)
    bs, bq, be = R.BOUNDS[fmt]
    for w in range(s.shape[0]):
        mi = Fraction(int(s[w, :, 0].sum()), 128) if remove_dc else 0
        mq = Fraction(int(s[w, :, 1].sum()), 128) if remove_dc else 0
        direct = 128 * sum((Fraction(int(i)) - mi) ** 2 + (Fraction(int(q)) - mq) ** 2 for i, q in s[w])
        assert direct == int(st["energy"][w])
        assert 0 <= int(st["energy"][w]) <= be and int(st["sum_sq"][w]) <= bq and abs(int(st["sum_i"][w])) <= bs and abs(int(st["sum_q"][w])) <= bs
    ext = R.stats(_extremes(fmt), fmt, 128, remove_dc)
    assert int(ext["sum_sq"][0]) == bq and int(ext["sum_i"][0]) == -bs                # all minimum: the bounds are attained
    assert int(ext["energy"][0]) == (0 if remove_dc else be) and int(ext["energy"][4]) == 0
    if remove_dc:
        assert int(ext["energy"][2]) == int(ext["energy"].max())                       # alternating: the largest centred E
    assert R.power_dbfs(ext["energy"].max(), fmt) <= 10 * np.log10(2.0) + 1e-12          # +3 dB at the most
    x = R.frames(_extremes(fmt), fmt, 1.0, 128, remove_dc)
    assert np.isfinite(x).all() and not x[4].any() and (not x[0].any()) == remove_dc


@pytest.mark.parametrize("fmt", ["ci8", "ci16"])
def test_reference_rms_equals_level_and_dc_offset_changes_nothing(fmt):
    amp = R.AMPLITUDE[fmt] // 2
    iq = _capture(fmt, 5, 256 * 50, -amp, amp)
    for level in (7.8e-3, 1.0, 3.0e4):
        for dc in (True, False):
            x = R.frames(iq, fmt, level, 128, dc)
            assert np.abs(np.sqrt((x * x).sum(axis=(1, 2)) / 128.0) / level - 1.0).max() <= 1e-12
    shifted = iq.copy().reshape(-1, 2)
    shifted[:, 0] += 17
    shifted[:, 1] -= 29
    shifted = shifted.reshape(-1)
    a, b = R.stats(iq, fmt), R.stats(shifted, fmt)
    np.testing.assert_array_equal(a["energy"], b["energy"])
    np.testing.assert_array_equal(b["sum_i"] - a["sum_i"], 128 * 17)
    np.testing.assert_array_equal(b["sum_q"] - a["sum_q"], -128 * 29)
    np.testing.assert_array_equal(R.emulate_f32_chain(iq, fmt, 7.8e-3), R.emulate_f32_chain(shifted, fmt, 7.8e-3))
    assert not np.array_equal(R.frames(iq, fmt, remove_dc=False), R.frames(shifted, fmt, remove_dc=False))


def test_reference_cross_format_identities():
    """What power-of-two scaling of the defined chain implies, on the f32 emulation of that chain -- bit for bit:
    u8 bytes XOR 0x80 read as int8 are s_u8 = 2 s_i8 + 1 (a DC offset and a factor 2); int8 << 8 read as int16 is a factor 256."""
    u8 = _capture("cu8", 7, 2 * (128 + 16 * 300))
    i8 = (u8 ^ 0x80).view(np.int8)
    for level in (7.8e-3, 1.0, 3.0e4):
        np.testing.assert_array_equal(R.emulate_f32_chain(u8, "cu8", level, 16).view(np.uint32), R.emulate_f32_chain(i8, "ci8", level, 16).view(np.uint32))
    a, b = R.stats(u8, "cu8", 16), R.stats(i8, "ci8", 16)
    np.testing.assert_array_equal(a["energy"], 4 * b["energy"])
    i16 = (i8.astype(np.int16) * 256).astype("<i2")
    for dc in (True, False):
        np.testing.assert_array_equal(R.emulate_f32_chain(i8, "ci8", 7.8e-3, 16, dc).view(np.uint32),
                                      R.emulate_f32_chain(i16, "ci16", 7.8e-3, 16, dc).view(np.uint32))
        a, b = R.stats(i8, "ci8", 16, dc), R.stats(i16, "ci16", 16, dc)
        np.testing.assert_array_equal(b["sum_i"], 256 * a["sum_i"])
        np.testing.assert_array_equal(b["sum_q"], 256 * a["sum_q"])
        np.testing.assert_array_equal(b["sum_sq"], 65536 * a["sum_sq"])
        np.testing.assert_array_equal(b["energy"], 65536 * a["energy"])


@pytest.mark.parametrize("fmt", ["ci8", "ci16"])
@pytest.mark.parametrize("remove_dc", [True, False])
def test_f32_chain_stays_within_the_derived_bound_of_the_f64_reference(fmt, remove_dc):
    """The chain the header makes normative, emulated in float32: within 2^-21 relative of the f64 reference (the bound the GPU
    test holds the kernels to), exactly 0 where the centred sample or E is 0."""
    iq = np.concatenate([_extremes(fmt), _capture(fmt, 8, 2 * (128 + 37 * 200)), _capture(fmt, 9, 256 * 40, -3, 4)])
    for level in (7.8e-3, 1.0, 3.0e4):
        x = R.emulate_f32_chain(iq, fmt, level, 37, remove_dc)
        x64 = R.frames(iq, fmt, level, 37, remove_dc)
        assert np.isfinite(x).all()
        assert (np.abs(x.astype(np.float64) - x64) <= 2.0 ** -21 * np.abs(x64)).all()
        zero = (R.centred(iq, fmt, 37, remove_dc) == 0) | (R.stats(iq, fmt, 37, remove_dc)["energy"] == 0)[:, None, None]
        assert (x[zero] == 0).all()


@pytest.mark.parametrize("fmt", ["ci8", "ci16"])
def test_reference_plain_conversion_and_quantiser(fmt):
    iq = _capture(fmt, 10, 2 * (128 + 37 * 5))
    x = R.plain_frames(iq, fmt, 1.0 / R.AMPLITUDE[fmt], 37)
    assert x.dtype == np.float32 and x.shape == (6, 2, 128) and np.abs(x).max() <= 1.0
    np.testing.assert_array_equal(x[2, 0], iq[2 * 37 * 2:2 * 37 * 2 + 256:2].astype(np.float64) / R.AMPLITUDE[fmt])      # a power of two: exact
    fr = np.random.default_rng(11).standard_normal((5, 2, 128)) * 0.01
    q = R.quantise_frames(fr, fmt, 100, (3, -2))
    assert q.dtype == R.DTYPE[fmt] and 97 <= np.abs(q.astype(np.int64)).max() <= 103
    back = R.frames(q, fmt, 1.0)
    ref = fr - fr.mean(axis=2, keepdims=True)
    ref /= np.sqrt((ref ** 2).sum(axis=(1, 2), keepdims=True) / 128)
    assert np.abs(back - ref).max() < 0.05
