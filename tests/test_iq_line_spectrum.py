"""The line spectrum and the estimators built on it, without a GPU (include/mdc.h: mdc_iq_line_spectrum; frontend.line_spectrum,
find_line, estimate_symbol_rate, estimate_carrier_offset):

  1. the float64 reference (tests/iq_line_ref.py) on full-scale on-bin tones: one line where and as high as the definition says,
     on the right side of 0;
  2. the corner pairs of every format against Python integers;
  3. find_line: the parabola, the one- and two-sided bands, its fall-backs;
  4. the estimators' rules on the reference spectra of the synthetic band's three emitters, isolated as VTCNN2.scan_iq(refine=True)
     isolates them;
  5. the argument errors of the new frontend functions;
  6. every refusal of mdc_iq_line_spectrum, before any device call."""
import ctypes
import functools

import numpy as np
import pytest

import iq_ddc_ref as D
import iq_line_ref as R
import iq_spectrum_ref as S
from modulationdetectioncnn_amd import _cabi, frontend


def _einval(rc, *words):
    msg = _cabi.lib().mdc_last_error().decode()
    assert rc == -22, (rc, msg)
    for w in words:
        assert w in msg, (w, msg)


# ------------------------------------------------------------------------------------------------------------ 1. reference sanity
@pytest.mark.parametrize("k", [5, 37, 100, -9])
def test_reference_puts_an_on_bin_tone_where_the_definition_says(k):
    """x = A e^{2 pi i k n / N} with A = 32767 (rounded to integers): y of order m is about A^m e^{2 pi i m k n / N}, so with a
    window of ones the only line is bin m k mod N, of power scale (N A^m 2^-q)^2; order 0 gives A^2 at DC.  The rounding of the
    samples (1/2 LSB of 32767) spreads a relative m 2^-16 in amplitude: the line within 1e-3, everything else 70 dB below."""
    N, A = 128, 32767.0
    n = np.arange(N)
    z = A * np.exp(2j * np.pi * k * n / N)
    iq = np.rint(np.stack([z.real, z.imag], axis=1)).astype("<i2").reshape(-1)
    ones = np.ones(N, np.int16)
    assert frontend.line_spectrum.__doc__ and R.ORDERS == _cabi.LINE_SPECTRUM_ORDERS
    for order, m in ((0, 0), (1, 1), (2, 2), (4, 4)):
        P = R.segment_powers(iq, "ci16", order, N, ones, 1.0, [0])[0]
        amp = A ** (order if order else 2) * 2.0 ** -R.Q[order]
        line = (m * k) % N                                       # +f stays +f: a conjugated square would land on -m k mod N
        assert int(np.argmax(P)) == line, (order, k)
        assert abs(P[line] / (N * amp) ** 2 - 1.0) < 1e-3, (order, k, P[line])
        rest = np.delete(P, line)
        assert rest.max() < 1e-7 * P[line], (order, k, rest.max() / P[line])


# ------------------------------------------------------------------------------------------------------------ 2. corner pairs
def _int_power(i, q, order):
    """Python integers: no width to overflow"""
    if order == 0:
        return i * i + q * q, 0
    if order == 1:
        return i, q
    a, b = i * i - q * q, 2 * i * q
    return (a, b) if order == 2 else (a * a - b * b, 2 * a * b)


def test_corner_pairs_are_python_integers():
    seen_min4 = False
    for fmt in ("cu8", "ci8", "ci16"):
        lo, hi = S.SAMPLE_MIN[fmt], S.SAMPLE_MAX[fmt]
        corners = [(lo, lo), (lo, hi), (hi, lo), (hi, hi), (lo, 0 if fmt != "cu8" else 128), (hi, lo + 1)]
        iq = np.array(corners, D.DTYPE[fmt]).reshape(-1)
        I, Q = D.widen(iq, fmt)
        for order in R.ORDERS:
            re, im = R.power_of(I, Q, order)
            assert re.dtype == np.int64 and im.dtype == np.int64
            for j in range(len(corners)):
                want = _int_power(int(I[j]), int(Q[j]), order)
                assert (int(re[j]), int(im[j])) == want, (fmt, order, corners[j])
                assert max(abs(want[0]), abs(want[1])) <= R.Y_MAX[order]
        if fmt == "ci16":                                        # I = Q = -32768: the square is (0, 2^31), its square (-2^62, 0)
            assert _int_power(-32768, -32768, 2) == (0, 2 ** 31) and _int_power(-32768, -32768, 0) == (2 ** 31, 0)
            re4, im4 = R.power_of(I[:1], Q[:1], 4)
            assert (int(re4[0]), int(im4[0])) == (-2 ** 62, 0)
            seen_min4 = True
            # the staged values of that corner under the largest window value: exactly representable, |v| <= 2^30
            w = np.array([32767], np.int64)
            assert R._times_window(re4, w, 48)[0] == -float(2 ** 62 * 32767) * 2.0 ** -48
            assert abs(R._times_window(R.power_of(I[:1], Q[:1], 2)[1], w, 16)[0]) == 2.0 ** 15 * 32767 <= 2.0 ** 30
    assert seen_min4


def test_reference_split_product_is_the_integer_product():
    """order 4's y w needs up to 77 bits: the split sum against Python's integers, to one float64 rounding"""
    rng = np.random.default_rng(0)
    y = np.concatenate([rng.integers(-2 ** 62, 2 ** 62, size=200), [-2 ** 62, 2 ** 62, 2 ** 37, -2 ** 37 - 1, 0, 1]]).astype(np.int64)
    w = rng.integers(-32768, 32768, size=y.size).astype(np.int64)
    got = R._times_window(y, w, 48)
    for g, a, b in zip(got, y, w):
        exact = int(a) * int(b)
        assert abs(g * 2.0 ** 48 - exact) <= abs(exact) * 2.0 ** -52, (a, b)


# ------------------------------------------------------------------------------------------------------------ 3. find_line
def _hann_line(nfft, position, level=1.0, floor=0.0):
    """power spectrum of a tone at `position` bins (fractional) under the periodic Hann window, plus a flat floor"""
    n = np.arange(nfft)
    w = 0.5 - 0.5 * np.cos(2 * np.pi * n / nfft)
    X = np.fft.fft(w * np.exp(2j * np.pi * position * n / nfft))
    return level * np.abs(X) ** 2 + floor


def _hann_lobe(d):
    """amplitude of the periodic Hann window's transform d bins from the tone, large nfft: sinc(d) / (1 - d^2), its limit 1/2 at
    |d| = 1"""
    d = np.asarray(d, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.sinc(d) / (1.0 - d * d)
    return np.where(np.isclose(np.abs(d), 1.0), 0.5, v)


def test_find_line_refines_a_hann_line_to_its_fractional_bin():
    """The log-parabola is exact for a Gaussian lobe.  For the Hann window's lobe sinc(d) / (1 - d^2) its answer has a closed form:
    find_line must give it (to 1e-4 bin: nfft is finite and the spectrum has a floor), it is exact on a bin and half way between
    two, and nowhere more than 0.016 bin off (largest about 0.28 bin from a bin)."""
    nfft, worst = 1024, 0.0
    for frac in np.linspace(-0.5, 0.5, 41):
        pos = 100 + frac
        f, db = frontend.find_line(_hann_line(nfft, pos, floor=1e-3), 0.05, 0.2)
        k = 100 if abs(frac) < 0.5 else int(np.rint(f * nfft))                              # at +-0.5 either neighbour is the peak
        a, b, c = (2.0 * np.log(_hann_lobe(k + o - pos)) for o in (-1, 0, 1))
        assert abs(f * nfft - (k + 0.5 * (a - c) / (a - 2 * b + c))) < 1e-4, frac
        worst = max(worst, abs(f * nfft - pos))
        assert db > 60.0
    print(f"largest error of the parabola on a Hann line: {worst:.4f} bins")
    assert worst <= 0.0165
    f, _ = frontend.find_line(_hann_line(nfft, 100.0, floor=1e-3), 0.05, 0.2)
    assert abs(f * nfft - 100.0) < 1e-6
    f, _ = frontend.find_line(_hann_line(nfft, -60.3, floor=1e-3), -0.1, -0.01)              # a negative frequency, natural order
    assert abs(f * nfft + 60.3) <= 0.0165


def test_find_line_bands_prominence_and_fall_backs():
    nfft = 64
    p = np.ones(nfft)
    p[10], p[nfft - 20] = 100.0, 400.0                                                       # +10/64 and the stronger -20/64
    f, db = frontend.find_line(p, 0.0, 0.49)
    assert f == 10 / nfft and abs(db - 20.0) < 1e-9                                           # one-sided: only f >= 0; a lone bin: delta = 0
    f, db = frontend.find_line(p, 0.0, 0.49, two_sided=True)
    assert f == -20 / nfft and abs(db - 10 * np.log10(400.0)) < 1e-9
    f, db = frontend.find_line(p, 0.2, 0.25, two_sided=True)                                  # neither line: bins 13..16 on both sides
    assert abs(f) >= 0.2 and db == 0.0
    f, _ = frontend.find_line(p, -0.4, -0.2)
    assert f == -20 / nfft
    # the band's edges are inclusive, and the median is over the searched bins only
    f, db = frontend.find_line(p, 10 / nfft, 10 / nfft)
    assert f == 10 / nfft and db == 0.0
    # the parabola: a = c gives delta 0, a > c pulls towards the bin before
    q = np.ones(nfft)
    q[29:32] = [4.0, 16.0, 4.0]
    assert frontend.find_line(q, 0.3, 0.6)[0] == 30 / nfft
    q[29:32] = [8.0, 16.0, 4.0]
    a, b, c = np.log(8.0), np.log(16.0), np.log(4.0)
    assert abs(frontend.find_line(q, 0.3, 0.6)[0] - (30 + 0.5 * (a - c) / (a - 2 * b + c)) / nfft) < 1e-15
    assert frontend.find_line(q, 0.3, 0.6)[0] < 30 / nfft
    # fall-backs: a neighbour <= 0, and no maximum (a plateau: a - 2b + c = 0)
    q[29:32] = [0.0, 16.0, 4.0]
    assert frontend.find_line(q, 0.4, 0.5)[0] == 30 / nfft
    flat = np.full(nfft, 3.0)
    f, db = frontend.find_line(flat, 0.1, 0.2)
    assert f == 7 / nfft and db == 0.0                                                       # the first of equals, delta = 0
    # circular neighbours: a line on bin 0 sees bin nfft - 1
    z = np.ones(nfft)
    z[0], z[1], z[nfft - 1] = 16.0, 4.0, 8.0
    assert frontend.find_line(z, 0.0, 0.1)[0] < 0.0
    # the last bin of natural order is -1/nfft; nfft/2 is -0.5, two-sided |f| = 0.5
    z = np.ones(nfft)
    z[nfft // 2] = 9.0
    assert frontend.find_line(z, 0.45, 0.5, two_sided=True)[0] == -0.5
    with pytest.raises(ValueError):
        frontend.find_line(p, 0.501, 0.6)
    with pytest.raises(ValueError):
        frontend.find_line(p, 0.3, 0.2)
    with pytest.raises(ValueError):
        frontend.find_line(p, 0.1001, 0.1002)                                                # between two bins
    with pytest.raises(ValueError):
        frontend.find_line(np.array([1.0, np.nan, 1.0, 1.0]), 0.0, 0.5)


# ------------------------------------------------------------------------------------------------------------ 4. the estimators' rules
NFFT, AVG, MIN_DB = 1024, 8, 8.0


@functools.lru_cache(maxsize=None)
def _isolated():
    """the three emitters of synthetic_band(1) found on the reference spectrum and isolated by the reference DDC, as
    VTCNN2.scan_iq(refine=True) does on the device: [(emitter, D0, iso int16 flat)]"""
    iq = S.synthetic_band(1)
    w = frontend.design_window(NFFT)
    found = frontend.find_emitters(S.band_psd(iq, NFFT, w, frontend.window_scale(w)), window=w)
    out = []
    for e in found:
        D0 = min(max(int(1.0 / (4.0 * e.bandwidth)), 1), 256)
        iso = D.ddc(iq, "ci16", 0, frontend.phase_step(-e.centre), D0, frontend.plan_taps(1, D0))
        out.append((e, D0, iso.reshape(-1)))
    return out


def _psd(iso, order):
    w = frontend.design_window(NFFT)
    return R.line_psd(iso, "ci16", order, NFFT, AVG, w, frontend.window_scale(w))


def test_estimators_rules_on_the_reference_spectra_of_the_band():
    """Measured on the reference (float64, this test's print), for 96 / 48 / 20 samples per symbol (D0 = 16 / 8 / 3): symbol
    line 34.7 / 31.8 / 19.0 dB, 0.0069 / 0.0056 / 0.0039 bins from D0 / sps; x^4 line 21.9 / 22.3 / 21.4 dB, centre + offset
    within 1.8e-7 / 1.9e-7 / 9.3e-7 of the truth (the centroid alone: 1.1e-5 / 3.4e-5 / 7.0e-5); the largest x^2 bin of the
    search band 2.9 / 1.6 / 0.9 dB over its median."""
    emitters = _isolated()
    assert len(emitters) == 3
    for (e, D0, iso), sps, fc, want in zip(emitters, S.BAND_SPS, S.BAND_CENTRES, ((1, 12), (1, 6), (2, 5))):
        b = e.bandwidth * D0
        assert D0 == int(1.0 / (4.0 * e.bandwidth)) and (b <= 0.25 or D0 == 1)
        rate, rate_db = frontend.find_line(_psd(iso, 0), b / 2.5, min(0.45, 1.25 * b))
        bins_off = abs(rate - D0 / sps) * NFFT
        f2, db2 = frontend.find_line(_psd(iso, 2), 0.0, 2 * b / 8.0, two_sided=True)
        f4, db4 = frontend.find_line(_psd(iso, 4), 0.0, 4 * b / 8.0, two_sided=True)
        carrier = e.centre + f4 / 4.0 / D0
        print(f"sps {sps}: D0 {D0}, symbol line {rate_db:.1f} dB, {bins_off:.4f} bins off; x^2 {db2:.1f} dB; x^4 {db4:.1f} dB, "
              f"carrier error {abs(carrier - fc):.2e} (centroid {abs(e.centre - fc):.2e})")
        assert bins_off <= 0.1
        assert frontend.resample_ratio(1.0, rate / D0, 8)[:2] == want
        assert db2 < MIN_DB                                      # QPSK: no line in the square, so the order chosen is 4
        assert db4 >= MIN_DB + 6.0 and rate_db >= MIN_DB + 6.0   # every accepted line clears the threshold by 6 dB
        assert abs(carrier - fc) <= 5e-6


# ------------------------------------------------------------------------------------------------------------ 5. argument errors
def test_frontend_argument_errors():
    iq = np.zeros(4096, np.int16)
    for order in (3, 8, -1, 5, True, None, "2"):
        with pytest.raises(ValueError, match="order"):
            frontend.line_spectrum(iq, "ci16", order)
    for lo, hi in ((0.0, 0.2), (-0.1, 0.2), (0.3, 0.2), (0.1, 0.51), (float("nan"), 0.2)):
        with pytest.raises(ValueError, match="band"):
            frontend.estimate_symbol_rate(iq, "ci16", lo, hi)
    for m in (0.0, -0.01, 0.125, 0.2, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="max_offset"):
            frontend.estimate_carrier_offset(iq, "ci16", m)
    with pytest.raises(ValueError):
        frontend.line_spectrum(iq, "cf32", 2)                    # an unknown sample format, before anything touches a device
    assert _cabi.IQ_LINE_ENVELOPE == 0 and "mdc_iq_line_spectrum" in _cabi.EXPORTS


# ------------------------------------------------------------------------------------------------------------ 6. the C entry point
def test_every_refusal_comes_before_any_device_call():
    L = _cabi.lib()
    assert hasattr(L, "mdc_iq_line_spectrum")
    buf = (ctypes.c_uint8 * 4096)()                              # host memory is fine: every check comes before a launch
    base = (ctypes.addressof(buf) + 63) // 64 * 64
    iq, win, out = base, base + 1024, base + 2048

    def call(fmt=_cabi.IQ_CI16, pairs=200, order=2, nfft=64, hop=32, avg=2, iq=iq, win=win, scale=1.0, out=out, rows=2):
        return L.mdc_iq_line_spectrum(iq, fmt, pairs, order, nfft, hop, avg, win, scale, out, rows, None)

    assert S.rows_count(200, 64, 32, 2) == 2
    for order in (3, 8, -1, 5, 6, 16):
        _einval(call(order=order), "mdc_iq_line_spectrum", "order")
    for order in R.ORDERS:
        _einval(call(order=order, fmt=7), "format")
        _einval(call(order=order, nfft=96), "nfft")
        _einval(call(order=order, nfft=32), "nfft")
        _einval(call(order=order, nfft=8192), "nfft")
        _einval(call(order=order, hop=0), "hop")
        _einval(call(order=order, avg=0), "avg")
        _einval(call(order=order, avg=4097), "avg")
        _einval(call(order=order, pairs=-1), "negative")
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            _einval(call(order=order, scale=bad), "scale")
        _einval(call(order=order, rows=3), "mdc_iq_line_spectrum", "rows", "mdc_iq_spectrogram_rows gives 2")
        _einval(call(order=order, rows=0), "rows")
        _einval(call(order=order, iq=iq + 2), "iq_dev", "4-byte")
        _einval(call(order=order, fmt=_cabi.IQ_CU8, iq=iq + 1), "iq_dev", "2-byte")
        _einval(call(order=order, fmt=_cabi.IQ_CI8, iq=iq + 1), "iq_dev", "2-byte")
        _einval(call(order=order, out=out + 2), "power_dev", "4-byte")
        _einval(call(order=order, win=win + 1), "window_dev", "2-byte")
        _einval(call(order=order, iq=None), "null buffer")
        _einval(call(order=order, win=None), "null buffer")
        _einval(call(order=order, out=None), "null buffer")
        # rows == 0: nothing to launch, whatever the buffers
        assert call(order=order, pairs=63, rows=0, iq=None, win=None, out=None) == 0
        assert call(order=order, pairs=0, rows=0) == 0
