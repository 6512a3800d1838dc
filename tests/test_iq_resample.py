"""The rational resampler (include/mdc.h: mdc_iq_resample, mdc_iq_resample_out_count; frontend.design_resampler, resample_ratio,
resample_out_count, resample) without a GPU: the count, the argument checks -- every one raised before any device call, so they
run on a machine without a device --, the filter design and its response, the choice of L / D, and the numpy reference itself
on a tone and on the extremes."""
import numpy as np
import pytest

import iq_resample_ref as R
from modulationdetectioncnn_amd import _cabi, frontend

EINVAL = -22
NAMES = ("mdc_iq_resample", "mdc_iq_resample_out_count")
DESIGNS = [(1, 4), (2, 3), (3, 2), (5, 6), (4, 5), (5, 12), (8, 25), (10, 3), (32, 33), (25, 48), (32, 1), (3, 125), (7, 128), (32, 128)]


def test_exports_and_abi_version():
    assert set(NAMES) <= set(_cabi.EXPORTS)
    assert _cabi.lib().mdc_abi_version() == 5
    for variant in ("product", "alternates"):
        for name in NAMES:
            assert hasattr(_cabi.lib(variant), name), (variant, name)
    assert (_cabi.RESAMPLE_MAX_INTERPOLATE, _cabi.RESAMPLE_MAX_DECIMATE, _cabi.RESAMPLE_MAX_TAPS, _cabi.RESAMPLE_MAX_BRANCH_ABS_SUM) == \
        (R.MAX_INTERPOLATE, R.MAX_DECIMATE, R.MAX_TAPS, R.MAX_BRANCH_ABS_SUM)


def _brute_count(P, T, L, D):
    """the outputs j >= 0 whose last sample j D + T - 1 still lies in the zero-stuffed capture of (P - 1) L + 1 samples"""
    lv = (P - 1) * L + 1 if P >= 1 else 0
    return len(range(0, lv - T + 1, D)) if lv >= T else 0


@pytest.mark.parametrize("L,D,T", [(1, 1, 1), (2, 3, 5), (5, 6, 48), (32, 1, 1024), (3, 256, 1024), (5, 6, 3)])
def test_out_count(L, D, T):
    lib = _cabi.lib()
    first = -(-(T - 1) // L) + 1                      # the smallest P with (P - 1) L + 1 >= T: one output
    second = -(-(T + D - 1) // L) + 1                 # ... >= T + D: two
    for P in (0, 1, first - 1, first, second - 1, second):
        want = _brute_count(P, T, L, D)
        assert lib.mdc_iq_resample_out_count(P, T, L, D) == want == R.out_count(P, T, L, D), (P, want)
        assert frontend.resample_out_count(P, T, L, D) == want
    assert R.out_count(first - 1, T, L, D) == 0 and R.out_count(first, T, L, D) >= 1 and R.out_count(second, T, L, D) >= 2
    big = ((10 ** 12 - 1) * L + 1 - T) // D + 1
    assert lib.mdc_iq_resample_out_count(10 ** 12, T, L, D) == big == R.out_count(10 ** 12, T, L, D)


def _einval(rc, *needles):
    assert rc == EINVAL, rc
    msg = _cabi.lib().mdc_last_error().decode()
    for needle in needles:
        assert needle in msg, msg


def test_out_count_argument_errors():
    lib = _cabi.lib()
    _einval(lib.mdc_iq_resample_out_count(100, 8, 0, 2), "interpolate")
    _einval(lib.mdc_iq_resample_out_count(100, 8, 33, 2), "interpolate")
    _einval(lib.mdc_iq_resample_out_count(100, 8, 2, 0), "decimate")
    _einval(lib.mdc_iq_resample_out_count(100, 8, 2, 257), "decimate")
    _einval(lib.mdc_iq_resample_out_count(100, 0, 2, 3), "ntaps")
    _einval(lib.mdc_iq_resample_out_count(100, 1025, 2, 3), "ntaps")
    _einval(lib.mdc_iq_resample_out_count(-1, 8, 2, 3), "negative")
    with pytest.raises(_cabi.MdcError):
        frontend.resample_out_count(100, 8, 33, 2)


def test_resample_argument_errors_come_before_any_device_call():
    """Fictitious device addresses: nothing may touch them (and this machine may have no device at all)."""
    lib = _cabi.lib()
    h = np.array([16384, 16384, 16384, 16384], np.int16)
    IN, OUT = 0x10000, 0x20000
    P, T, L, D = 100, 4, 2, 3
    n = R.out_count(P, T, L, D)
    assert n > 0

    def call(iq=IN, fmt=_cabi.IQ_CI16, pairs=P, L=L, D=D, taps=h, T=T, out=OUT, n_out=n):
        return lib.mdc_iq_resample(iq, fmt, pairs, 0, 0, L, D, taps.ctypes.data if taps is not None else None, T, out, n_out, None)

    _einval(call(fmt=3), "format")
    _einval(call(fmt=-1), "format")
    _einval(call(L=0), "interpolate")
    _einval(call(L=33), "interpolate")
    _einval(call(D=0), "decimate")
    _einval(call(D=257), "decimate")
    _einval(call(T=0), "ntaps")
    _einval(call(T=1025), "ntaps")
    _einval(call(pairs=-1), "negative")
    _einval(call(taps=None), "null taps")
    big = np.array([1, 32767, 1, -32767, 1, 2], np.int16)            # branch 1 of L = 2: 32767 + 32767 + 2 = 65536
    assert R.branch_abs_sums(big, 2) == [3, 65536]
    _einval(call(taps=big, T=6, n_out=R.out_count(P, 6, L, D)), "branch 1", "65536")
    with pytest.raises(AssertionError):
        R.check_taps(big, 2)
    _einval(call(n_out=n + 1), "n_out")
    _einval(call(n_out=n - 1), "n_out")
    _einval(call(n_out=0), "n_out")
    _einval(call(iq=None), "null")
    _einval(call(out=None), "null")
    _einval(call(iq=IN + 2), "pair")                                 # CI16: pairs are 4 bytes
    _einval(call(iq=IN + 1, fmt=_cabi.IQ_CU8), "pair")
    _einval(call(iq=IN + 1, fmt=_cabi.IQ_CI8), "pair")
    _einval(call(out=OUT + 2), "4-byte")
    # nothing to do is not an error: a capture shorter than the filter, no buffers at all
    assert R.out_count(2, T, L, D) == 0
    assert lib.mdc_iq_resample(None, _cabi.IQ_CU8, 2, 0, 0, L, D, h.ctypes.data, T, None, 0, None) == 0
    assert lib.mdc_iq_resample(None, _cabi.IQ_CU8, 0, 0, 0, L, D, h.ctypes.data, T, None, 0, None) == 0
    # the bound holds per BRANCH: a prototype of sum |h| = 131,070, each of its two branches at 65,535, passes the tap check
    # (and then fails on n_out)
    ok = np.array([32767, -32767, -32767, 32767, 1, -1], np.int16)
    assert R.branch_abs_sums(ok, 2) == [65535, 65535] and int(np.abs(ok.astype(np.int64)).sum()) == 131070
    _einval(call(taps=ok, T=6, n_out=-5), "n_out")
    # ... while the same taps as ONE branch (L = 1) are refused
    _einval(call(L=1, taps=ok, T=6, n_out=R.out_count(P, 6, 1, D)), "branch 0", "131070")


def test_frontend_resample_argument_errors():
    iq = np.zeros(64, np.uint8)
    with pytest.raises(ValueError, match="explicit taps"):
        frontend.resample(iq, "cu8", interpolate=1, decimate=1)
    with pytest.raises(ValueError, match="explicit taps"):
        frontend.resample(iq, "cu8", interpolate=6, decimate=6)
    with pytest.raises(TypeError):
        frontend.resample(iq, "cu8", interpolate=2, decimate=3, taps=np.array([0.5, 0.5]))
    with pytest.raises(ValueError):
        frontend.resample(iq, "cu8", interpolate=2, decimate=3, taps=np.array([40000, 1]))
    with pytest.raises(ValueError):
        frontend.resample(iq, "cu8", shift=0.7, interpolate=2, decimate=3)
    with pytest.raises(ValueError, match="interpolate"):
        frontend.resample(iq, "cu8", interpolate=33, decimate=3)
    with pytest.raises(ValueError, match="decimate"):
        frontend.resample(iq, "cu8", interpolate=2, decimate=0)


@pytest.mark.parametrize("L,D", DESIGNS)
def test_design_resampler(L, D):
    """dtype, every branch's sum 32768, every branch's sum |h| <= 65535, and the two figures design_lowpass promises, at the
    interpolated rate: droop <= 0.95 dB over |f| <= 0.25 / M, >= 63 dB for |f| >= 0.75 / M.  (A numpy restatement of the design
    gave, over these fourteen pairs: droop 0.80 .. 0.90 dB, stopband 68.2 .. 81.6 dB, largest branch sum |h| 42,272.)  ntaps is
    min(8 M, 1024): the default wherever 8 M stays below the limit, explicit where it reaches it."""
    M = max(L, D)
    T = min(8 * M, 1024)
    h = frontend.design_resampler(L, D) if 8 * M < 1024 else frontend.design_resampler(L, D, ntaps=T)
    assert h.dtype == np.int16 and h.shape == (T,)
    h64 = h.astype(np.int64)
    assert [int(h64[r::L].sum()) for r in range(L)] == [32768] * L
    sums = R.branch_abs_sums(h, L)
    assert max(sums) <= 65535
    R.check_taps(h, L)
    N = 1 << 18
    H = np.abs(np.fft.fft(h.astype(np.float64) / (32768.0 * L), N))
    f = np.fft.fftfreq(N)
    with np.errstate(divide="ignore"):
        db = 20.0 * np.log10(H)
    droop = -db[np.abs(f) <= 0.25 / M].min()
    stop = -db[np.abs(f) >= 0.75 / M].max()
    print(f"L/D {L}/{D}: {T} taps, largest branch sum|h| {max(sums)}, droop {droop:.3f} dB, stopband {stop:.1f} dB")
    assert droop <= 0.95
    assert stop >= 63.0


def test_design_resampler_arguments():
    for D in (2, 4, 12):
        np.testing.assert_array_equal(frontend.design_resampler(1, D), frontend.design_lowpass(D))
    np.testing.assert_array_equal(frontend.design_resampler(1, 4, ntaps=33, cutoff=0.11, beta=6.0), frontend.design_lowpass(4, 33, 0.11, 6.0))
    assert frontend.design_resampler(5, 6, ntaps=47).shape == (47,)
    with pytest.raises(ValueError, match="ntaps"):
        frontend.design_resampler(3, 200)                            # 8 M = 1600 taps: the caller has to choose
    assert frontend.design_resampler(3, 200, ntaps=1024).shape == (1024,)
    for bad in (dict(interpolate=0, decimate=2), dict(interpolate=33, decimate=2), dict(interpolate=2, decimate=0), dict(interpolate=2, decimate=257),
                dict(interpolate=1, decimate=1), dict(interpolate=2, decimate=3, ntaps=0), dict(interpolate=2, decimate=3, ntaps=1025),
                dict(interpolate=2, decimate=3, cutoff=0.0), dict(interpolate=2, decimate=3, cutoff=0.6),
                dict(interpolate=8, decimate=1, ntaps=3)):           # branches of one tap of ~3 x 87,000: outside int16
        with pytest.raises(ValueError):
            frontend.design_resampler(**bad)


def test_resample_ratio():
    assert frontend.resample_ratio(2.4e6, 250e3) == (5, 6, 8.0)
    assert frontend.resample_ratio(2.048e6, 200e3) == (25, 32, 8.0)
    assert frontend.resample_ratio(1e6, 125e3) == (1, 1, 8.0)
    assert frontend.resample_ratio(1e6, 250e3) == (2, 1, 8.0)               # below 8 samples per symbol: L > D
    assert frontend.resample_ratio(2.4e6, 250e3, samples_per_symbol=4) == (5, 12, 4.0)
    L, D, sps = frontend.resample_ratio(2.4e6, 270833.0)                    # GSM's symbol rate: no exact ratio
    assert L <= 32 and D <= 256 and abs(sps / 8.0 - 1.0) <= 0.01 and np.gcd(L, D) == 1
    with pytest.raises(ValueError, match="1 %"):
        frontend.resample_ratio(1e6, 100.0)                                 # 1/1250: the smallest ratio is 1/256
    with pytest.raises(ValueError, match="1 %"):
        frontend.resample_ratio(2.4e6, 250e3, max_interpolate=4, max_decimate=4)      # 5/6 is out of reach; 3/4, 1/1 are 10 % off
    with pytest.raises(ValueError):
        frontend.resample_ratio(0.0, 250e3)


def test_reference_on_a_tone():
    """A CU8 capture of amplitude 100 (of 127.5) at f0 = 0.2 with an interferer of amplitude 20, shifted by -0.2 and resampled by
    5/6: what remains is a constant of magnitude 100 * 2 * 128 = 25,600 (the widening's gain; every branch has DC gain exactly 1),
    within 0.2 %.
    The interferer sits at f0 + 0.5, the farthest the input band allows: at the interpolated rate the input's own Nyquist
    frequency is 0.5 / L = 0.1, below the stopband edge 0.75 / M = 0.125, so NO component of a capture can reach the stopband in
    its baseband image -- that is the stretch between the output's passband and what aliases onto it, which a resampler close
    to 1 does not have to reject; the stopband proper holds the IMAGES of the zero stuffing.  At 0.1 the filter is 29 dB down.
    Measured with the reference: magnitude 25,631.7, residual standard deviation 269.0 LSB (without the interferer 25,623.0 and
    85.7: the byte quantisation, -49.5 dBc, of which a 5/6 resampler passes two thirds -- the DDC's decimation by 12 leaves 0.9).
    Asserted with a margin of 1.5."""
    L, D, n = 5, 6, 6 * 4000
    t = np.arange(n)
    z = 100.0 * np.exp(2j * np.pi * (0.2 * t + 1.0 / np.pi)) + 20.0 * np.exp(2j * np.pi * (0.7 * t + 1.0 / np.e))
    iq = np.clip(np.rint(np.stack([z.real, z.imag], axis=1) + 127.5), 0, 255).astype(np.uint8).reshape(-1)
    h = frontend.design_resampler(L, D)
    out = R.resample(iq, "cu8", 0, frontend.phase_step(-0.2), L, D, h).astype(np.float64)
    assert out.shape == (R.out_count(n, h.size, L, D), 2)
    w = out[:, 0] + 1j * out[:, 1]
    mag = float(np.abs(w.mean()))
    resid = float(np.sqrt(np.mean(np.abs(w - w.mean()) ** 2)))
    print(f"magnitude {mag:.1f}, residual standard deviation {resid:.3f} LSB")
    assert abs(mag - 25600.0) <= 0.002 * 25600.0
    assert resid < 1.5 * 269.0


def test_reference_is_the_ddc_reference_for_one_branch():
    import iq_ddc_ref as DR
    rng = np.random.default_rng(3)
    iq = rng.integers(-128, 128, size=2 * 700).astype(np.int8)
    h = frontend.design_lowpass(3, ntaps=16)
    np.testing.assert_array_equal(R.resample(iq, "ci8", 123456789, 987654321, 1, 3, h), DR.ddc(iq, "ci8", 123456789, 987654321, 3, h))
    picks = [0, 5, 100, R.out_count(700, 29, 5, 6) - 1]
    g = frontend.design_resampler(5, 6, ntaps=29)
    np.testing.assert_array_equal(R.resample_sparse(iq, "ci8", 7, 1 << 30, 5, 6, g, picks), R.resample(iq, "ci8", 7, 1 << 30, 5, 6, g)[picks])


def test_reference_asserts_its_ranges_on_the_extremes():
    """All-minimum CI16 at the phases where the mixer's sum is largest, through random-sign taps with EVERY branch at
    sum |h| = 65535: the reference's own range assertions (|m| <= 32767, |acc| + 8192 < 2^31) hold; a branch of 65536 is refused."""
    iq = np.full(2 * 64, -32768, np.dtype("<i2"))
    rng = np.random.default_rng(5)
    L, D = 3, 2
    h = np.full(24, 8191, np.int64)
    h[:3] += 65535 - 8 * 8191                                   # one tap per branch takes the rest
    assert R.branch_abs_sums(h, L) == [65535] * 3
    h *= rng.choice([-1, 1], size=24)
    for phase0 in (0, 1 << 29, 5 << 29, 3 << 30):
        out = R.resample(iq, "ci16", phase0, 0, L, D, h.astype(np.int16))
        assert out.shape == (R.out_count(64, 24, L, D), 2)
    one = np.array([16384, 16384, 16384, 16384], np.int16)      # two branches of DC gain exactly 1
    np.testing.assert_array_equal(R.resample(iq, "ci16", 5 << 29, 0, 2, 1, one)[:2], [(0, 32767)] * 2)      # clamped from 46,340
    np.testing.assert_array_equal(R.resample(iq, "ci16", 0, 0, 2, 1, one)[:2], [(-32766, -32766)] * 2)
    with pytest.raises(AssertionError):
        R.resample(iq, "ci16", 0, 0, 2, 1, np.array([32767, 1, -32767, 1, 2], np.int16))       # branch 0: 65536
