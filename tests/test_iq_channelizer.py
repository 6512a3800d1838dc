"""The channelizer without a GPU (include/mdc.h: mdc_iq_channelizer, mdc_iq_channelizer_out_count; frontend.design_channelizer,
channelizer_out_count, channel_freqs, channelize's host-tap validation):

  1. the symbols, the output count against the formula, and every argument refusal of both entry points, before any device call;
  2. design_channelizer's documented figures from its own taps (dense FFT) for M in {8, 16, 64, 256, 1024}, and its refusals;
  3. the float64 reference (tests/iq_channelizer_ref.py) against the exact-integer down-converter's reference (tests/iq_ddc_ref.py)
     channel by channel: two independent restatements of "shift by -k/M, low-pass, decimate" agree within 2 LSB."""
import ctypes

import numpy as np
import pytest

import iq_channelizer_ref as R
import iq_ddc_ref as D
from modulationdetectioncnn_amd import _cabi, frontend

NAMES = ("mdc_iq_channelizer", "mdc_iq_channelizer_out_count")


def _einval(rc, *words):
    msg = _cabi.lib().mdc_last_error().decode()
    assert rc == -22, (rc, msg)
    for w in words:
        assert w in msg, (w, msg)


# ------------------------------------------------------------------------------------------------------------ 1. the C entry points
def test_symbols_are_declared_bound_and_exported():
    assert set(NAMES) <= set(_cabi.EXPORTS)
    L = _cabi.lib()
    for name in NAMES:
        assert hasattr(L, name), name
    assert _cabi.ABI_VERSION == 5 and L.mdc_abi_version() == 5 and _cabi.CHANNELIZER_GRID_CAP >= 1
    assert (_cabi.CHANNELIZER_MIN_CHANNELS, _cabi.CHANNELIZER_MAX_CHANNELS, _cabi.CHANNELIZER_MAX_TAPS_PER_CHANNEL,
            _cabi.CHANNELIZER_MAX_TAP_SHIFT, _cabi.CHANNELIZER_MAX_BRANCH_ABS_SUM) == (8, 1024, 16, 15, 65535)
    assert [_cabi.channelizer_tile_steps(m) for m in (8, 16, 64, 128, 1024)] == [128, 64, 16, 16, 16]


def test_out_count_is_the_formula():
    L = _cabi.lib()
    for M in (8, 64, 1024):
        for Dm in (1, 3, M // 2, M):
            for T in (1, M - 3, M, 3 * M + 5, 8 * M, 16 * M):
                for pairs in (0, 1, T - 1, T, T + 1, T + Dm - 1, T + Dm, T + 36 * Dm, T + 36 * Dm + Dm - 1, 1 << 20, (1 << 40) + 12345):
                    want = (pairs - T) // Dm + 1 if pairs >= T else 0
                    assert L.mdc_iq_channelizer_out_count(pairs, M, T, Dm) == want == R.out_count(pairs, T, Dm)
                    assert frontend.channelizer_out_count(pairs, M, T, Dm) == want
    for bad in (0, 4, 12, 100, 2048, -8):
        _einval(L.mdc_iq_channelizer_out_count(1000, bad, 8, 1), "channels")
    _einval(L.mdc_iq_channelizer_out_count(1000, 16, 8, 0), "decimate")
    _einval(L.mdc_iq_channelizer_out_count(1000, 16, 8, 17), "decimate")
    _einval(L.mdc_iq_channelizer_out_count(1000, 16, 0, 8), "ntaps")
    _einval(L.mdc_iq_channelizer_out_count(1000, 16, 257, 8), "ntaps")
    _einval(L.mdc_iq_channelizer_out_count(-1, 16, 8, 8), "negative")
    with pytest.raises(_cabi.MdcError):
        frontend.channelizer_out_count(1000, 12, 8, 1)


def test_every_refusal_comes_before_any_device_call():
    L = _cabi.lib()
    buf = (ctypes.c_uint8 * 8192)()                       # host memory is fine: every check comes before a launch
    base = (ctypes.addressof(buf) + 63) // 64 * 64
    iq, taps, out = base, base + 2048, base + 4096

    def call(fmt=_cabi.IQ_CI16, pairs=200, first=0, M=16, Dm=8, taps=taps, T=128, shift=3, iq=iq, out=out, n_out=10):
        return L.mdc_iq_channelizer(iq, fmt, pairs, first, M, Dm, taps, T, shift, out, n_out, None)

    assert R.out_count(200, 128, 8) == 10
    _einval(call(fmt=7), "format")
    for bad in (0, 4, 12, 24, 2048):
        _einval(call(M=bad), "channels")
    _einval(call(Dm=0), "decimate")
    _einval(call(Dm=17), "decimate")
    _einval(call(T=0), "ntaps")
    _einval(call(T=257), "ntaps")
    _einval(call(shift=-1), "tap_shift")
    _einval(call(shift=16), "tap_shift")
    _einval(call(pairs=-1), "negative")
    _einval(call(first=-1), "first_index")
    _einval(call(n_out=11), "n_out", "mdc_iq_channelizer_out_count gives 10")
    _einval(call(n_out=0), "n_out")
    _einval(call(iq=iq + 2), "iq_dev", "4-byte")
    _einval(call(fmt=_cabi.IQ_CU8, iq=iq + 1), "iq_dev", "2-byte")
    _einval(call(fmt=_cabi.IQ_CI8, iq=iq + 1), "iq_dev", "2-byte")
    _einval(call(taps=taps + 1), "taps_dev", "2-byte")
    _einval(call(out=out + 2), "out_dev", "4-byte")
    _einval(call(iq=None), "null buffer")
    _einval(call(taps=None), "null buffer")
    _einval(call(out=None), "null buffer")
    # n_out == 0: nothing to launch, whatever the buffers
    assert call(pairs=127, n_out=0, iq=None, taps=None, out=None) == 0
    assert call(pairs=0, n_out=0) == 0


# ------------------------------------------------------------------------------------------------------------ 2. the prototype filter
@pytest.mark.parametrize("M", [8, 16, 64, 256, 1024])
def test_design_channelizer_figures_from_its_taps(M):
    h, shift = frontend.design_channelizer(M)
    assert h.dtype == np.int16 and h.shape == (8 * M,) and shift == int(np.log2(M)) - 1
    q = h.astype(np.int64)
    assert int(q.sum()) == 32768 << shift and np.array_equal(q, q[::-1])
    worst_residue = max(int(np.abs(q[r::M]).sum()) for r in range(M))
    assert worst_residue <= _cabi.CHANNELIZER_MAX_BRANCH_ABS_SUM
    R.check_taps(h, M)
    N = 1 << 20                                                        # dense: 1024 .. 2^17 points per channel spacing
    f = np.fft.fftfreq(N)
    db = 20.0 * np.log10(np.maximum(np.abs(np.fft.fft(q.astype(np.float64), N)) / float(32768 << shift), 1e-30))
    droop = -db[np.abs(f) <= 0.25 / M].min()
    edge = db[np.argmin(np.abs(f - 0.5 / M))]
    att = -db[np.abs(f) >= 0.85 / M].max()
    print(f"M {M}: droop {droop:.4f} dB, edge {edge:.3f} dB, attenuation {att:.2f} dB, largest tap {q.max()}, largest residue {worst_residue}")
    assert droop <= 0.1 and db[np.abs(f) <= 0.25 / M].max() <= 1e-6
    assert abs(edge + 6.0) <= 0.1
    assert att >= 75.0
    assert abs(int(q.max()) - 16380) <= 150 and abs(worst_residue - 24600) <= 350      # "about": M = 8 has the coarsest sampling of the pulse


def test_design_channelizer_and_channelize_refuse_bad_taps():
    for bad in (0, 4, 12, 2048):
        with pytest.raises(ValueError):
            frontend.design_channelizer(bad)
    with pytest.raises(ValueError):
        frontend.design_channelizer(16, taps_per_channel=0)
    with pytest.raises(ValueError):
        frontend.design_channelizer(16, taps_per_channel=17)
    with pytest.raises(ValueError):
        frontend.design_channelizer(16, cutoff=0.0)
    with pytest.raises(ValueError):
        frontend.design_channelizer(16, cutoff=0.6)
    with pytest.raises(ValueError):
        frontend.design_channelizer(16, taps_per_channel=1, cutoff=0.5)      # 16 taps of a near-impulse: the centre taps leave int16
    h, shift = frontend.design_channelizer(16, taps_per_channel=4, cutoff=0.02, beta=5.0)
    assert h.size == 64 and shift == 3 and int(h.astype(np.int64).sum()) == 32768 << 3
    # channelize's host-tap validation (frontend._check_channelizer_taps): everything the library cannot check of a device buffer
    check = frontend._check_channelizer_taps
    good = check(np.array([20000, -20000, 5] * 9, np.int64), 8)
    assert good.dtype == np.int16 and good.size == 27
    with pytest.raises(TypeError):
        check(np.ones(8, np.float32), 8)
    with pytest.raises(TypeError):
        check(np.ones((2, 8), np.int16), 8)
    with pytest.raises(ValueError):
        check(np.zeros(0, np.int16), 8)
    with pytest.raises(ValueError):
        check(np.ones(16 * 8 + 1, np.int16), 8)
    with pytest.raises(ValueError):
        check(np.array([40000] * 8, np.int32), 8)
    over = np.zeros(24, np.int16)
    over[[3, 11, 19]] = (30000, -30000, 5536)                                   # residue 3: 65,536
    with pytest.raises(ValueError, match="residue 3"):
        check(over, 8)
    over[19] = 5535                                                             # 65,535: allowed
    check(over, 8)
    np.testing.assert_array_equal(frontend.channel_freqs(8), [0, 0.125, 0.25, 0.375, -0.5, -0.375, -0.25, -0.125])
    with pytest.raises(ValueError):
        frontend.channel_freqs(12)


# ------------------------------------------------------------------------------------------------------------ 3. two restatements agree
def test_reference_agrees_with_the_exact_down_converter_channel_by_channel():
    """M = 64, D = 32, Q15 taps (s = 0), T = 512, uniform full-range ci16 input: rint of the channelizer reference against
    iq_ddc_ref.ddc with step = (-k 2^32 / M) mod 2^32 and phase0 = first_index * step.  The down-converter rounds its oscillator to
    a 12-bit table of 15-bit values and its mixer to int16 (half the product), the channelizer reference rounds nothing: the
    unrounded difference is below 1 LSB, so the rounded outputs differ by at most 2."""
    M, Dm, T, first = 64, 32, 512, 5
    taps = frontend.design_lowpass(Dm, ntaps=T, cutoff=0.5 / M)
    assert int(taps.astype(np.int64).sum()) == 32768
    rng = np.random.default_rng(11)
    pairs = T + 40 * Dm
    iq = rng.integers(-32768, 32768, size=2 * pairs).astype(np.dtype("<i2"))
    Y, S = R.channelize(iq, "ci16", first, M, Dm, taps, 0)
    assert Y.shape == (M, 41) and S.shape == (41,)
    got = R.rounded(Y).astype(np.int64)
    worst, worst_unrounded = 0, 0.0
    for k in range(M):
        step = (-k * (1 << 32) // M) % (1 << 32)
        want = D.ddc(iq, "ci16", (first * step) % (1 << 32), step, Dm, taps).astype(np.int64)
        worst = max(worst, int(np.abs(got[k] - want).max()))
        inside = np.abs(want) < 32767                                                  # unrounded difference where nothing clamps
        re, im = R.clamped(Y[k])
        worst_unrounded = max(worst_unrounded, float(np.abs(np.stack([re, im], axis=1) - want)[inside].max()) - 0.5)
    print(f"largest |rint(reference) - ddc| {worst} LSB; unrounded, beyond the ddc's own final rounding: {worst_unrounded:.3f} LSB")
    assert worst <= 2
