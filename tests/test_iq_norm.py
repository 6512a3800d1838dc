"""Level-normalised raw I/Q windows (include/mdc.h, mdc_iq_u8_windows_norm / mdc_predict_host_iq_u8_norm) without a GPU:
the two entry points validate their arguments before any device call, and the numpy restatement the GPU tests hold the
kernel to (tests/iq_norm_ref.py) has the properties the header states."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import iq_norm_ref as R
from modulationdetectioncnn_amd import _cabi, frontend


def test_norm_entry_points_validate_their_arguments_without_gpu():
    L = _cabi.lib()
    L.mdc_last_error.restype = ctypes.c_char_p
    buf = (ctypes.c_uint8 * 1024)()
    out = (ctypes.c_uint8 * 4096)()
    iq = ctypes.addressof(buf)
    x = (ctypes.addressof(out) + 15) & ~15
    DC = _cabi.IQ_REMOVE_DC
    f = L.mdc_iq_u8_windows_norm
    assert f(iq, -1, 128, 1.0, DC, x, None, None) == -22 and b"negative" in L.mdc_last_error()
    assert f(None, 2, 128, 1.0, DC, x, None, None) == -22 and b"null input" in L.mdc_last_error()
    assert f(iq, 2, 128, 1.0, DC, None, None, None) == -22 and b"both null" in L.mdc_last_error()
    for level in (0.0, -1.0, float("nan"), float("inf")):
        assert f(iq, 2, 128, level, DC, x, None, None) == -22 and b"level" in L.mdc_last_error(), level
    assert f(iq, 2, 128, 1.0, 2, x, None, None) == -22 and b"flag" in L.mdc_last_error()
    assert f(iq, 2, 128, 1.0, DC | 4, x, None, None) == -22 and b"flag" in L.mdc_last_error()
    for hop in (0, -3, (1 << 24) + 1):
        assert f(iq, 2, hop, 1.0, DC, x, None, None) == -22 and b"hop" in L.mdc_last_error(), hop
    assert f(iq + 1, 2, 16, 1.0, DC, x, None, None) == -22 and b"2-byte" in L.mdc_last_error()
    assert f(iq, 2, 16, 1.0, DC, x + 4, None, None) == -22 and b"8-byte" in L.mdc_last_error()
    assert f(iq, 2, 16, 1.0, DC, None, x + 8, None) == -22 and b"16-byte" in L.mdc_last_error()
    assert f(None, 0, 16, 1.0, 0, x, None, None) == 0                      # n = 0: nothing to launch
    h = L.mdc_predict_host_iq_u8_norm
    assert h(None, iq, 2, 128, 1.0, DC, None, None, None, 0) == -22 and b"null model" in L.mdc_last_error()
    assert h(None, iq, 2, 128, 0.0, DC, None, None, None, 0) == -22 and b"level" in L.mdc_last_error()
    assert h(None, iq, 2, 128, float("nan"), DC, None, None, None, 0) == -22 and b"level" in L.mdc_last_error()
    assert h(None, iq, 2, 128, 1.0, 8, None, None, None, 0) == -22 and b"flag" in L.mdc_last_error()
    assert h(None, iq, 2, 0, 1.0, DC, None, None, None, 0) == -22 and b"hop" in L.mdc_last_error()


def test_binding_describes_the_stats_record():
    assert _cabi.IQ_WINDOW_STATS.itemsize == 16 and _cabi.IQ_WINDOW_STATS == R.STATS_DTYPE
    assert {"mdc_iq_u8_windows_norm", "mdc_predict_host_iq_u8_norm"} <= set(_cabi.EXPORTS)
    assert _cabi.ABI_VERSION == 5


def _capture(seed, nbytes, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, size=nbytes, dtype=np.uint8)


@pytest.mark.parametrize("hop", [128, 16, 37])
@pytest.mark.parametrize("remove_dc", [True, False])
def test_reference_rms_equals_level(hop, remove_dc):
    iq = _capture(3, 2 * (128 + hop * 99))
    for level in (7.8e-3, 1.0, 250.0):
        x = R.frames(iq, level, hop, remove_dc)
        assert x.shape == (100, 2, 128)
        rms = np.sqrt((x * x).sum(axis=(1, 2)) / 128.0)
        assert np.abs(rms / level - 1.0).max() <= 1e-12


@pytest.mark.parametrize("remove_dc", [True, False])
def test_reference_energy_is_the_exact_centred_sum(remove_dc):
    iq = _capture(4, 2 * (128 + 37 * 19))
    st = R.stats(iq, 37, remove_dc)
    s = R.windows(iq, 37)
    for w in range(s.shape[0]):
        mi = Fraction(int(s[w, :, 0].sum()), 128) if remove_dc else 0
        mq = Fraction(int(s[w, :, 1].sum()), 128) if remove_dc else 0
        direct = 128 * sum((Fraction(int(i)) - mi) ** 2 + (Fraction(int(q)) - mq) ** 2 for i, q in s[w])
        assert direct == int(st["energy"][w])
        assert 0 <= int(st["energy"][w]) <= 128 * 256 * 255 ** 2


def test_reference_is_invariant_under_a_dc_offset():
    iq = _capture(5, 256 * 50, 40, 200)
    shifted = iq.copy().reshape(-1, 2)
    shifted[:, 0] += 17
    shifted[:, 1] -= 29
    shifted = shifted.reshape(-1)
    a, b = R.stats(iq), R.stats(shifted)
    np.testing.assert_array_equal(a["energy"], b["energy"])
    np.testing.assert_array_equal(b["sum_i"] - a["sum_i"], 2 * 128 * 17)
    np.testing.assert_array_equal(b["sum_q"] - a["sum_q"], -2 * 128 * 29)
    np.testing.assert_array_equal(R.frames(iq), R.frames(shifted))          # a is exact and E equal: bit-identical in f64 too
    assert not np.array_equal(R.frames(iq, remove_dc=False), R.frames(shifted, remove_dc=False))


def test_reference_constant_window_is_all_zero():
    iq = np.concatenate([np.full(256, 0, np.uint8), np.full(256, 255, np.uint8), np.tile(np.array([3, 250], np.uint8), 128)])
    x = R.frames(iq)
    assert np.isfinite(x).all() and not x.any()
    np.testing.assert_array_equal(R.stats(iq)["energy"], 0)
    assert (R.stats(iq, remove_dc=False)["energy"] > 0).all()
    assert np.isneginf(R.power_dbfs(R.stats(iq)["energy"])).all()


def test_power_and_squelch_threshold_agree_with_the_reference():
    e = np.array([0, 1, 1065369, 1065370, R.FULL_SCALE_ENERGY, 2130739200], np.int64)
    rec = np.zeros(e.size, _cabi.IQ_WINDOW_STATS)
    rec["energy"] = e
    np.testing.assert_array_equal(frontend.window_power_dbfs(rec), R.power_dbfs(e))
    assert frontend.window_power_dbfs(rec)[4] == 0.0 and np.isneginf(frontend.window_power_dbfs(rec)[0])
    cols = np.zeros((e.size, 4), np.int32)
    cols[:, 3] = e
    np.testing.assert_array_equal(frontend.window_power_dbfs(cols), R.power_dbfs(e))
    energies = np.unique(np.concatenate([e, np.random.default_rng(6).integers(0, 2130739201, size=4000)]))
    for sq in (-60.0, -30.0, -12.5, 0.0, 3.0, 10.0, float("-inf")):
        thr = frontend.squelch_energy_threshold(sq)
        np.testing.assert_array_equal(energies < thr, R.power_dbfs(energies) < sq)


def test_predict_iq_u8_refuses_contradicting_arguments():
    from modulationdetectioncnn_amd import VTCNN2
    m = VTCNN2.synthetic("deployed3")
    iq = np.zeros(512, np.uint8)
    with pytest.raises(ValueError, match="scale"):
        m.predict_iq_u8(iq, scale=0.01, normalize="rms")
    with pytest.raises(ValueError, match="normalize"):
        m.predict_iq_u8(iq, normalize="peak")
    with pytest.raises(ValueError, match="normalize='rms'"):
        m.predict_iq_u8(iq, squelch_dbfs=-30.0)
    with pytest.raises(ValueError, match="normalize='rms'"):
        m.predict_iq_u8(iq, return_power=True)
