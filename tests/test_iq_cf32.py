"""Float captures without a device: the numpy restatement (tests/iq_cf32_ref.py) on hand-made edges, frontend.design_cf32_gain
against it and against what it promises (nothing kept clips, 13 to 14 bits are used), every argument error of
mdc_iq_cf32_histogram / mdc_iq_cf32_quantize (MDC_EINVAL and a fitting mdc_last_error() before any device call), the binding,
and quantize_cf32's own argument checks.  The kernels are held to the restatement in tests/test_iq_cf32_gpu.py."""
import ctypes

import numpy as np
import pytest

import iq_cf32_ref as R
from modulationdetectioncnn_amd import _cabi, frontend
from modulationdetectioncnn_amd import cf32_histogram, design_cf32_gain, quantize_cf32      # noqa: F401  (exported from the package)


# ------------------------------------------------------------------------------------------------------------------ the reference
def test_reference_on_the_edges():
    out, bad, clipped = R.quantize(R.EDGES, R.EDGE_GAIN)
    np.testing.assert_array_equal(out, R.EDGES_OUT)
    assert (bad, clipped) == (0, R.EDGES_CLIPPED)
    # one by one, what the list is there for
    q = lambda v: R.quantize(np.array([v, 0.0], np.float32), 32768.0)      # noqa: E731
    assert [int(q(k / 32768.0)[0][0]) for k in (0.5, 1.5, 2.5, -0.5, -1.5, -2.5)] == [0, 2, 2, 0, -2, -2]      # ties to even
    assert (int(q(32767.5 / 32768)[0][0]), q(32767.5 / 32768)[2]) == (32767, 1)
    assert (int(q(-32768.5 / 32768)[0][0]), q(-32768.5 / 32768)[2]) == (-32768, 0)
    assert (int(q(1.0)[0][0]), q(1.0)[2]) == (32767, 1) and (int(q(-1.0)[0][0]), q(-1.0)[2]) == (-32768, 0)
    assert (int(q(3e38)[0][0]), q(3e38)[1:]) == (32767, (0, 1)) and (int(q(-3e38)[0][0]), q(-3e38)[1:]) == (-32768, (0, 1))
    assert (int(q(1e-45)[0][0]), q(1e-45)[1:]) == (0, (0, 0))
    # a denormal stays below 0.5 at the largest gain
    assert R.quantize(np.array([np.float32(2.0 ** -126) - np.float32(2.0 ** -149), 0], np.float32), 2.0 ** 125)[0][0] == 0


def test_reference_zeroes_and_counts_nonfinite_pairs():
    x = np.array([1, np.nan, np.inf, 2, 3, -np.inf, np.nan, np.nan, 4, 5, 40000, 6], np.float32)
    out, bad, clipped = R.quantize(x, 1.0)
    np.testing.assert_array_equal(out, [0, 0, 0, 0, 0, 0, 0, 0, 4, 5, 32767, 6])
    assert (bad, clipped) == (4, 1)
    h = R.histogram(x)
    assert h[255] == 5 and h.sum() == 12 and h[127] == 1 and h[128] == 2 and h[129] == 3 and h[142] == 1
    assert R.histogram(np.array([0.0, -0.0, 1e-45, -1e-39], np.float32))[0] == 4
    np.testing.assert_array_equal(R.histogram(x.view(np.complex64)), h)
    np.testing.assert_array_equal(R.histogram(x.reshape(-1, 2)), h)


# ---------------------------------------------------------------------------------------------------------------------- the design
@pytest.mark.parametrize("scale", [1e-3, 1.0, 3e4, 2.0 ** -20])
def test_design_resolves_noise_at_any_scale(scale):
    x = (scale * np.random.default_rng(5).standard_normal(8192)).astype(np.float32)
    h = R.histogram(x)
    gain = design_cf32_gain(h)
    assert gain == R.design_gain(h) and np.log2(gain) == int(np.log2(gain))
    out, bad, clipped = R.quantize(x, gain)
    assert (bad, clipped) == (0, 0)
    assert 2 ** 13 <= int(np.abs(out.astype(np.int32)).max()) < 2 ** 14


def test_design_gives_up_glitches_for_resolution():
    x = (1e-3 * np.random.default_rng(6).standard_normal(8192)).astype(np.float32)
    x[[100, 4000, 8000]] = [1e6, -1e6, 1e6]
    h = R.histogram(x)
    spoilt = design_cf32_gain(h)      # the plain maximum: the noise gets 2^14 * 1e-3 / 1e6 of an LSB
    assert np.abs(R.quantize(x, spoilt)[0][[0, 1, 2, 3]]).max() == 0
    gain = design_cf32_gain(h, clip_fraction=1e-3)
    assert gain == R.design_gain(h, 1e-3) and gain > spoilt * 2 ** 20
    out, bad, clipped = R.quantize(x, gain)
    assert (bad, clipped) == (0, 3)
    noise = np.delete(out.astype(np.int32), [100, 4000, 8000])
    assert 2 ** 13 <= np.abs(noise).max() < 2 ** 15 and noise.std() > 1000      # the bin in front of the top kept one still fits


def test_design_without_a_normal_component_is_one():
    assert design_cf32_gain(np.zeros(256, np.uint64)) == 1.0
    assert design_cf32_gain(R.histogram(np.array([0.0, 1e-45, -1e-40, 0.0], np.float32))) == 1.0
    assert design_cf32_gain(R.histogram(np.array([np.nan, np.inf], np.float32))) == 1.0
    # the clamp: a capture below 2^-111 takes the largest gain, and the largest float the smallest the walk can ask for
    assert design_cf32_gain(R.histogram(np.array([2.0 ** -120, 0.0], np.float32))) == 2.0 ** 125
    assert design_cf32_gain(R.histogram(np.array([3e38, 0.0], np.float32))) == 2.0 ** -114
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError):
            design_cf32_gain(np.zeros(256, np.uint64), clip_fraction=bad)
    with pytest.raises(ValueError):
        design_cf32_gain(np.zeros(255, np.uint64))


# ----------------------------------------------------------------------------------------------------------------------- the C ABI
def _lib():
    L = _cabi.lib()
    L.mdc_last_error.restype = ctypes.c_char_p
    return L


def test_binding():
    assert "mdc_iq_cf32_histogram" in _cabi.EXPORTS and "mdc_iq_cf32_quantize" in _cabi.EXPORTS and _cabi.ABI_VERSION == 5
    L = _lib()
    assert L.mdc_iq_cf32_histogram.argtypes[1] is ctypes.c_int64 and L.mdc_iq_cf32_quantize.argtypes[2] is ctypes.c_float
    assert (_cabi.CF32_GRID_CAP, _cabi.CF32_GROUP_PAIRS, _cabi.CF32_MAX_PAIRS) == (1024, 1024, 1 << 40)
    assert (_cabi.CF32_MIN_GAIN, _cabi.CF32_MAX_GAIN) == (R.MIN_GAIN, R.MAX_GAIN)


def test_histogram_entry_validates_its_arguments_without_gpu():
    L = _lib()
    buf = (ctypes.c_uint8 * 4096)()      # host memory is fine here: every check comes before any launch
    a = (ctypes.addressof(buf) + 15) & ~15
    assert L.mdc_iq_cf32_histogram(a, -1, a + 64, None) == -22 and b"negative" in L.mdc_last_error()
    assert L.mdc_iq_cf32_histogram(a, (1 << 40) + 1, a + 64, None) == -22 and b"2^40" in L.mdc_last_error()
    assert L.mdc_iq_cf32_histogram(a + 4, 1, a + 64, None) == -22 and b"iq_dev must be 8-byte aligned" in L.mdc_last_error()
    assert L.mdc_iq_cf32_histogram(a, 1, a + 68, None) == -22 and b"hist_dev must be 8-byte aligned" in L.mdc_last_error()
    assert L.mdc_iq_cf32_histogram(None, 1, a + 64, None) == -22 and b"null buffer" in L.mdc_last_error()
    assert L.mdc_iq_cf32_histogram(a, 1, None, None) == -22 and b"null buffer" in L.mdc_last_error()
    assert L.mdc_iq_cf32_histogram(None, 0, None, None) == 0
    assert L.mdc_iq_cf32_histogram(a + 8, 0, a + 64, None) == 0      # 8 bytes off a 16-byte boundary is a good address


def test_quantize_entry_validates_its_arguments_without_gpu():
    L = _lib()
    buf = (ctypes.c_uint8 * 4096)()
    a = (ctypes.addressof(buf) + 15) & ~15
    out, counts = a + 2048, a + 4000
    assert L.mdc_iq_cf32_quantize(a, -1, 1.0, out, counts, None) == -22 and b"negative" in L.mdc_last_error()
    assert L.mdc_iq_cf32_quantize(a, (1 << 40) + 1, 1.0, out, counts, None) == -22 and b"2^40" in L.mdc_last_error()
    for gain in (0.0, -1.0, float("nan"), float("inf"), 2.0 ** -127, 2.0 ** 126):
        assert L.mdc_iq_cf32_quantize(a, 1, gain, out, counts, None) == -22 and b"gain" in L.mdc_last_error(), gain
        assert L.mdc_iq_cf32_quantize(a, 0, gain, out, counts, None) == -22, gain      # also with nothing to do
    assert L.mdc_iq_cf32_quantize(a + 4, 1, 1.0, out, counts, None) == -22 and b"iq_dev must be 8-byte aligned" in L.mdc_last_error()
    assert L.mdc_iq_cf32_quantize(a, 1, 1.0, out + 2, counts, None) == -22 and b"output must be 4-byte aligned" in L.mdc_last_error()
    assert L.mdc_iq_cf32_quantize(a, 1, 1.0, out, counts + 4, None) == -22 and b"counts_dev must be 8-byte aligned" in L.mdc_last_error()
    assert L.mdc_iq_cf32_quantize(None, 1, 1.0, out, counts, None) == -22 and b"null buffer" in L.mdc_last_error()
    assert L.mdc_iq_cf32_quantize(a, 1, 1.0, None, counts, None) == -22 and b"null buffer" in L.mdc_last_error()
    # 100 pairs: 800 bytes in, 400 out -- the output's first byte on the input's last, and its last on the input's first
    assert L.mdc_iq_cf32_quantize(a + 400, 100, 1.0, a + 1196, None, None) == -22 and b"overlap" in L.mdc_last_error()
    assert L.mdc_iq_cf32_quantize(a + 400, 100, 1.0, a + 4, None, None) == -22 and b"overlap" in L.mdc_last_error()
    assert L.mdc_iq_cf32_quantize(a, 100, 1.0, a, None, None) == -22 and b"overlap" in L.mdc_last_error()
    for gain in (2.0 ** -126, 1.0, 32768 / 0.7, 2.0 ** 125):
        assert L.mdc_iq_cf32_quantize(None, 0, gain, None, None, None) == 0
        assert L.mdc_iq_cf32_quantize(a + 8, 0, gain, out + 4, counts, None) == 0


# ---------------------------------------------------------------------------------------------------------------- the Python layer
def test_quantize_cf32_checks_its_arguments_before_any_device_call():
    ok = np.zeros(8, np.float32)
    for bad in (np.zeros(8, np.float64), np.zeros(8, np.complex128), np.zeros(8, np.int16), np.zeros(8, np.float16)):
        with pytest.raises(TypeError):
            quantize_cf32(bad, full_scale=1.0)
        with pytest.raises(TypeError):
            cf32_histogram(bad)
    torch = pytest.importorskip("torch")
    with pytest.raises(TypeError):
        quantize_cf32(torch.zeros(8, dtype=torch.float64), full_scale=1.0)
    for bad in (np.zeros(7, np.float32), np.zeros((4, 3), np.float32), np.zeros((2, 2, 2), np.float32), np.zeros((4, 1), np.complex64)):
        with pytest.raises(ValueError):
            quantize_cf32(bad, full_scale=1.0)
    with pytest.raises(ValueError):
        quantize_cf32(ok, nonfinite="maybe")
    for p in (-0.01, 1.0, 1.5):
        with pytest.raises(ValueError):
            quantize_cf32(ok, clip_fraction=p)
    for fs in (0.0, -1.0, float("nan"), float("inf"), 1e-40, 3e38 * 1e6):
        with pytest.raises(ValueError):
            quantize_cf32(ok, full_scale=fs)
    # and cf32 is no fourth format of the integer entries
    with pytest.raises(ValueError):
        frontend.sample_format_id("cf32")
