"""The digital down-converter (include/mdc.h: mdc_iq_ddc, mdc_iq_ddc_out_count, mdc_iq_ddc_nco_table; frontend.phase_step,
design_lowpass, ddc) without a GPU: the oscillator table, the filter design and its response, the argument checks -- every one
raised before any device call, so they run on a machine without a device --, and the numpy reference itself on a tone."""
import ctypes as C

import numpy as np
import pytest

import iq_ddc_ref as R
from modulationdetectioncnn_amd import _cabi, frontend

DECIMATIONS = [2, 3, 4, 8, 12, 16, 32, 64]
EINVAL = -22


def test_exports_and_abi_version():
    assert {"mdc_iq_ddc", "mdc_iq_ddc_out_count", "mdc_iq_ddc_nco_table"} <= set(_cabi.EXPORTS)
    assert _cabi.lib().mdc_abi_version() == 5
    for variant in ("product", "alternates"):
        for name in ("mdc_iq_ddc", "mdc_iq_ddc_out_count", "mdc_iq_ddc_nco_table"):
            assert hasattr(_cabi.lib(variant), name), (variant, name)


def test_nco_table_is_the_reference_table():
    t = frontend.nco_table()
    assert t.dtype == np.int16 and t.shape == (4096, 2)
    np.testing.assert_array_equal(t, R.nco_table())
    assert tuple(t[0]) == (32767, 0) and tuple(t[1024]) == (0, 32767) and tuple(t[2048]) == (-32767, 0)
    with pytest.raises(_cabi.MdcError):
        _cabi.check(_cabi.lib().mdc_iq_ddc_nco_table(None))


def test_generator_reproduces_the_committed_table():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("gen_nco_table", os.path.join(root, "tools", "gen_nco_table.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    np.testing.assert_array_equal(gen.table(), R.nco_table())
    assert open(gen.PATH).read() == gen.text()


@pytest.mark.parametrize("D", DECIMATIONS)
def test_design_lowpass(D):
    h = frontend.design_lowpass(D)
    assert h.dtype == np.int16 and h.shape == (8 * D,)
    np.testing.assert_array_equal(h, h[::-1])
    s, a = int(h.astype(np.int64).sum()), int(np.abs(h.astype(np.int64)).sum())
    assert s == 32768
    assert a <= 65535
    assert a <= 40712, a                                     # the figure the documentation quotes
    N = 1 << 16
    H = np.abs(np.fft.fft(h.astype(np.float64) / 32768.0, N))
    f = np.fft.fftfreq(N)
    with np.errstate(divide="ignore"):
        db = 20.0 * np.log10(H)
    droop = -db[np.abs(f) <= 0.25 / D].min()
    stop = -db[np.abs(f) >= 0.75 / D].max()
    six = db[np.argmin(np.abs(f - 0.4 / D))]
    print(f"D {D}: sum|h| {a}, droop {droop:.3f} dB, stopband {stop:.1f} dB, response at 0.4/D {six:.2f} dB")
    assert droop <= 0.95
    assert stop >= 63.0
    assert abs(six + 6.02) < 0.25                            # the -6 dB point lies at the cutoff


def test_design_lowpass_arguments():
    assert frontend.design_lowpass(4, ntaps=33).shape == (33,)
    h = frontend.design_lowpass(4, ntaps=33)
    np.testing.assert_array_equal(h, h[::-1])
    assert int(h.astype(np.int64).sum()) == 32768
    for bad in (dict(decimate=1), dict(decimate=0), dict(decimate=4, ntaps=0), dict(decimate=4, ntaps=1025), dict(decimate=4, cutoff=0.0),
                dict(decimate=4, cutoff=0.6)):
        with pytest.raises(ValueError):
            frontend.design_lowpass(**bad)


def test_phase_step():
    assert frontend.phase_step(0.0) == 0
    assert frontend.phase_step(0.25) == 1 << 30
    assert frontend.phase_step(-0.25) == 3 << 30
    assert frontend.phase_step(-0.5) == 1 << 31
    assert frontend.phase_step(0.5) == 1 << 31
    assert frontend.phase_step(1e-10) == 0                  # 0.43 of one step: rounds to none
    assert frontend.phase_step(-0.2) == (1 << 32) - round(0.2 * 2 ** 32)
    for bad in (0.51, -0.6, float("nan")):
        with pytest.raises(ValueError):
            frontend.phase_step(bad)


@pytest.mark.parametrize("D,T", [(1, 1), (3, 16), (12, 96), (256, 1024)])
def test_out_count(D, T):
    L = _cabi.lib()
    for P, want in ((0, 0), (T - 1, 0), (T, 1), (T + D - 1, 1), (T + D, 2), (10 ** 12, (10 ** 12 - T) // D + 1)):
        assert L.mdc_iq_ddc_out_count(P, T, D) == want == R.out_count(P, T, D)
        assert frontend.ddc_out_count(P, T, D) == want


def _einval(rc, needle):
    assert rc == EINVAL, rc
    msg = _cabi.lib().mdc_last_error().decode()
    assert needle in msg, msg


def test_out_count_argument_errors():
    L = _cabi.lib()
    _einval(L.mdc_iq_ddc_out_count(100, 8, 0), "decimate")
    _einval(L.mdc_iq_ddc_out_count(100, 8, 257), "decimate")
    _einval(L.mdc_iq_ddc_out_count(100, 0, 2), "ntaps")
    _einval(L.mdc_iq_ddc_out_count(100, 1025, 2), "ntaps")
    _einval(L.mdc_iq_ddc_out_count(-1, 8, 2), "negative")


def test_ddc_argument_errors_come_before_any_device_call():
    """Fictitious device addresses: nothing may touch them (and this machine may have no device at all)."""
    L = _cabi.lib()
    h = np.array([16384, 16384, 0, 0], np.int16)
    IN, OUT = 0x10000, 0x20000
    P, T, D = 100, 4, 2
    n = R.out_count(P, T, D)

    def call(iq=IN, fmt=_cabi.IQ_CI16, pairs=P, D=D, taps=h, T=T, out=OUT, n_out=n):
        return L.mdc_iq_ddc(iq, fmt, pairs, 0, 0, D, taps.ctypes.data if taps is not None else None, T, out, n_out, None)

    _einval(call(fmt=3), "format")
    _einval(call(fmt=-1), "format")
    _einval(call(D=0), "decimate")
    _einval(call(D=257), "decimate")
    _einval(call(T=0), "ntaps")
    _einval(call(T=1025), "ntaps")
    _einval(call(pairs=-1), "negative")
    _einval(call(taps=None), "null taps")
    big = np.array([32767, -32767, 2], np.int16)             # sum |h| = 65536
    assert int(np.abs(big.astype(np.int64)).sum()) == 65536
    _einval(call(taps=big, T=3, n_out=R.out_count(P, 3, D)), "65536")
    _einval(call(n_out=n + 1), "n_out")
    _einval(call(n_out=n - 1), "n_out")
    _einval(call(n_out=0), "n_out")
    _einval(call(iq=None), "null")
    _einval(call(out=None), "null")
    _einval(call(iq=IN + 2), "pair")                         # CI16: pairs are 4 bytes
    _einval(call(iq=IN + 1, fmt=_cabi.IQ_CU8), "pair")
    _einval(call(iq=IN + 1, fmt=_cabi.IQ_CI8), "pair")
    _einval(call(out=OUT + 2), "4-byte")
    # nothing to do is not an error: a capture shorter than the filter, no buffers at all
    assert L.mdc_iq_ddc(None, _cabi.IQ_CU8, 3, 0, 0, D, h.ctypes.data, T, None, 0, None) == 0
    ok = np.array([32767, -32767, 1], np.int16)              # sum |h| = 65535 passes the tap check (and then fails on n_out)
    _einval(call(taps=ok, T=3, n_out=-5), "n_out")


def test_frontend_ddc_argument_errors():
    iq = np.zeros(64, np.uint8)
    with pytest.raises(ValueError, match="explicit taps"):
        frontend.ddc(iq, "cu8", decimate=1)
    with pytest.raises(TypeError):
        frontend.ddc(iq, "cu8", decimate=2, taps=np.array([0.5, 0.5]))
    with pytest.raises(ValueError):
        frontend.ddc(iq, "cu8", decimate=2, taps=np.array([40000, 1]))
    with pytest.raises(ValueError):
        frontend.ddc(iq, "cu8", shift=0.7, decimate=2)


def test_reference_on_a_tone():
    """A CU8 capture of amplitude 100 (of 127.5) at f0 = 0.2 with an interferer of amplitude 20 at f0 + 0.15, shifted by -0.2
    and decimated by 12: the interferer lands at 0.15 = 1.8 / D, in the stopband; what remains is a constant of magnitude
    100 * 2 * 128 = 25,600 (the widening's gain), within 0.2 %, with under one LSB of residual.  What is left is the output's
    own rounding (0.41 LSB for a complex value) and the harmonics of the BYTE quantisation that fall into the transition band:
    the capture repeats every 20 samples, so its quantisation error is a line spectrum, and which lines are strong depends on
    the tones' starting phases -- 0.5 to 1.4 LSB over a handful of phases tried, 11 LSB with both phases 0, where samples sit
    exactly on rounding ties.  The phases here are 1/pi and 1/e cycles (no sample near a tie): magnitude 25,581.3, residual 0.89."""
    D, n = 12, 12 * 4000
    t = np.arange(n)
    z = 100.0 * np.exp(2j * np.pi * (0.2 * t + 1.0 / np.pi)) + 20.0 * np.exp(2j * np.pi * (0.35 * t + 1.0 / np.e))
    iq = np.clip(np.rint(np.stack([z.real, z.imag], axis=1) + 127.5), 0, 255).astype(np.uint8).reshape(-1)
    h = frontend.design_lowpass(D)
    out = R.ddc(iq, "cu8", 0, frontend.phase_step(-0.2), D, h).astype(np.float64)
    assert out.shape == (R.out_count(n, h.size, D), 2)
    w = out[:, 0] + 1j * out[:, 1]
    mag = float(np.abs(w.mean()))
    resid = float(np.sqrt(np.mean(np.abs(w - w.mean()) ** 2)))
    print(f"magnitude {mag:.1f}, residual standard deviation {resid:.3f} LSB")
    assert abs(mag - 25600.0) <= 0.002 * 25600.0
    assert resid < 1.0


def test_reference_asserts_its_ranges_on_the_extremes():
    """All-minimum CI16 at the phases where the mixer's sum is largest, through random-sign taps of sum |h| = 65535: the
    reference's own range assertions (|m| <= 32767, |acc| + 8192 < 2^31) hold, and the outputs saturate as documented."""
    iq = np.full(2 * 64, -32768, np.dtype("<i2"))
    one = np.array([16384, 16384], np.int16)             # DC gain exactly 1
    np.testing.assert_array_equal(R.ddc(iq, "ci16", 5 << 29, 0, 1, one)[0], (0, 32767))           # clamped from 46,340
    np.testing.assert_array_equal(R.ddc(iq, "ci16", 1 << 29, 0, 1, one)[0], (0, -32768))
    np.testing.assert_array_equal(R.ddc(iq, "ci16", 0, 0, 1, one)[0], (-32766, -32766))
    rng = np.random.default_rng(5)
    h = np.full(16, 4095, np.int64)
    h[0] += 65535 - h.sum()
    h *= rng.choice([-1, 1], size=16)
    for phase0 in (0, 1 << 29, 5 << 29, 3 << 30):
        out = R.ddc(iq, "ci16", phase0, 0, 3, h.astype(np.int16))
        assert out.shape == (17, 2)
    with pytest.raises(AssertionError):
        R.ddc(iq, "ci16", 0, 0, 1, np.array([32767, -32767, 2], np.int16))
