"""The power spectrogram and the emitter scan without a GPU (include/mdc.h: mdc_iq_spectrogram, mdc_iq_spectrogram_rows;
frontend.spectrogram_rows, design_window, window_scale, window_enbw, spectrum_freqs, find_emitters, channel_plan):

  1. the row count against the formula, and every argument refusal of both entry points, before any device call;
  2. the window helpers against closed forms, the committed twiddle table against its formula;
  3. find_emitters / channel_plan on the float64 reference spectrum (tests/iq_spectrum_ref.py) of a synthetic band of three
     QPSK emitters: count, order, centres, bandwidths, powers, plans; noise alone; a lone DC spike."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import iq_spectrum_ref as S
from conftest import ROOT
from modulationdetectioncnn_amd import _cabi, frontend

NAMES = ("mdc_iq_spectrogram", "mdc_iq_spectrogram_rows")


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
    assert _cabi.ABI_VERSION == 5 and _cabi.SPECTROGRAM_GRID_CAP >= 1


def test_row_count_is_the_formula():
    L = _cabi.lib()
    for nfft in (64, 256, 4096):
        for hop in (1, 7, nfft // 2, nfft, nfft + 3, 5 * nfft):
            for avg in (1, 2, 3, 16, 4096):
                for pairs in (0, 1, nfft - 1, nfft, nfft + 1, nfft + hop - 1, nfft + hop, nfft + 7 * hop + 2, nfft + (3 * avg - 1) * hop,
                              nfft + (3 * avg - 1) * hop - 1, 1 << 20, (1 << 40) + 12345):
                    want = ((pairs - nfft) // hop + 1) // avg if pairs >= nfft else 0
                    assert L.mdc_iq_spectrogram_rows(pairs, nfft, hop, avg) == want == S.rows_count(pairs, nfft, hop, avg)
                    assert frontend.spectrogram_rows(pairs, nfft, hop, avg) == want
    _einval(L.mdc_iq_spectrogram_rows(1000, 100, 10, 1), "nfft")
    _einval(L.mdc_iq_spectrogram_rows(1000, 32, 10, 1), "nfft")
    _einval(L.mdc_iq_spectrogram_rows(1000, 8192, 10, 1), "nfft")
    _einval(L.mdc_iq_spectrogram_rows(1000, 0, 10, 1), "nfft")
    _einval(L.mdc_iq_spectrogram_rows(1000, 64, 0, 1), "hop")
    _einval(L.mdc_iq_spectrogram_rows(1000, 64, -5, 1), "hop")
    _einval(L.mdc_iq_spectrogram_rows(1000, 64, 10, 0), "avg")
    _einval(L.mdc_iq_spectrogram_rows(1000, 64, 10, 4097), "avg")
    _einval(L.mdc_iq_spectrogram_rows(-1, 64, 10, 1), "negative")
    with pytest.raises(_cabi.MdcError):
        frontend.spectrogram_rows(1000, 100, 10, 1)


def test_every_refusal_comes_before_any_device_call():
    L = _cabi.lib()
    buf = (ctypes.c_uint8 * 4096)()                       # host memory is fine: every check comes before a launch
    base = (ctypes.addressof(buf) + 63) // 64 * 64
    iq, win, out = base, base + 1024, base + 2048

    def call(fmt=_cabi.IQ_CI16, pairs=200, nfft=64, hop=32, avg=2, iq=iq, win=win, scale=1.0, out=out, rows=2):
        return L.mdc_iq_spectrogram(iq, fmt, pairs, nfft, hop, avg, win, scale, out, rows, None)

    assert S.rows_count(200, 64, 32, 2) == 2
    _einval(call(fmt=7), "format")
    _einval(call(nfft=96), "nfft")
    _einval(call(nfft=32), "nfft")
    _einval(call(nfft=8192), "nfft")
    _einval(call(hop=0), "hop")
    _einval(call(avg=0), "avg")
    _einval(call(avg=4097), "avg")
    _einval(call(pairs=-1), "negative")
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        _einval(call(scale=bad), "scale")
    _einval(call(rows=3), "rows", "mdc_iq_spectrogram_rows gives 2")
    _einval(call(rows=0), "rows")
    _einval(call(iq=iq + 2), "iq_dev", "4-byte")
    _einval(call(fmt=_cabi.IQ_CU8, iq=iq + 1), "iq_dev", "2-byte")
    _einval(call(fmt=_cabi.IQ_CI8, iq=iq + 1), "iq_dev", "2-byte")
    _einval(call(out=out + 2), "power_dev", "4-byte")
    _einval(call(win=win + 1), "window_dev", "2-byte")
    _einval(call(iq=None), "null buffer")
    _einval(call(win=None), "null buffer")
    _einval(call(out=None), "null buffer")
    # rows == 0: nothing to launch, whatever the buffers
    assert call(pairs=63, rows=0, iq=None, win=None, out=None) == 0
    assert call(pairs=64 + 32 * 2, avg=4, rows=0, iq=None, win=None, out=None) == 0          # three segments do not fill a row of four
    assert call(pairs=0, rows=0) == 0


# ------------------------------------------------------------------------------------------------------------ 2. window helpers
def test_window_helpers_against_closed_forms():
    for nfft in (64, 1024, 4096):
        w = frontend.design_window(nfft)
        assert w.dtype == np.int16 and w.shape == (nfft,) and w[0] == 0 and w[nfft // 2] == 32767 and w.min() >= 0
        assert np.abs(w[1:].astype(int) - w[1:][::-1]).max() <= 1                           # periodic: symmetric about nfft/2 (up to the rounding of x.5)
        np.testing.assert_array_equal(w, np.rint(32767 * (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(nfft) / nfft))).astype(np.int16))
        s1 = int(w.astype(np.int64).sum())
        assert abs(s1 - 32767 * nfft / 2) <= nfft / 2                                        # sum of the exact Hann is nfft/2; rounding: half an LSB each
        assert frontend.window_scale(w) == 1.0 / (32768.0 * s1) ** 2
        assert abs(frontend.window_scale(w) * (32768.0 * 32767.0 * nfft / 2) ** 2 - 1.0) < 1e-3
        assert abs(frontend.window_enbw(w) - 1.5) < 1e-3
        k = frontend.design_window(nfft, "kaiser", beta=6.0)
        kf = np.kaiser(nfft, 6.0)
        np.testing.assert_array_equal(k, np.rint(32767 * kf).astype(np.int16))
        assert abs(frontend.window_enbw(k) - nfft * (kf ** 2).sum() / kf.sum() ** 2) < 1e-3
        ones = np.full(nfft, 32767, np.int16)
        assert frontend.window_enbw(ones) == 1.0 and frontend.window_scale(ones) == 1.0 / (32768.0 * 32767 * nfft) ** 2
    with pytest.raises(ValueError):
        frontend.window_scale(np.zeros(64, np.int16))
    with pytest.raises(ValueError):
        frontend.window_scale(np.array([5, -5] * 32, np.int16))
    with pytest.raises(ValueError):
        frontend.window_enbw(np.zeros(64, np.int16))
    with pytest.raises(ValueError):
        frontend.design_window(64, "boxcar")


def test_spectrum_freqs():
    for nfft in (64, 1024):
        f = frontend.spectrum_freqs(nfft)
        assert f.shape == (nfft,) and f[0] == 0.0 and f[1] == 1.0 / nfft and f[nfft // 2 - 1] == 0.5 - 1.0 / nfft
        assert f[nfft // 2] == -0.5 and f[-1] == -1.0 / nfft and f.min() >= -0.5 and f.max() < 0.5
        np.testing.assert_array_equal(f, np.where(np.arange(nfft) < nfft // 2, np.arange(nfft), np.arange(nfft) - nfft) / nfft)


def test_committed_twiddles_are_the_formula():
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_fft_twiddles.py"), "--check"]).returncode == 0


# ------------------------------------------------------------------------------------------------------------ 3. the scan
@pytest.fixture(scope="module")
def band_psds():
    out = {}
    for seed in (1, 2, 3):
        iq = S.synthetic_band(seed)
        for nfft in (1024, 4096):
            w = frontend.design_window(nfft)
            out[seed, nfft] = (S.band_psd(iq, nfft, w, frontend.window_scale(w)), w)
    return out


@pytest.mark.parametrize("nfft", [1024, 4096])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_three_emitters_are_found_and_planned(band_psds, seed, nfft):
    psd, w = band_psds[seed, nfft]
    found = frontend.find_emitters(psd, window=w)
    print([tuple(round(v, 5) for v in e) for e in found], [frontend.channel_plan(e.centre, e.bandwidth)[1:3] for e in found])
    assert len(found) == 3
    assert [e.centre for e in found] == sorted(e.centre for e in found)
    for e, sps, fc, amp in zip(found, S.BAND_SPS, S.BAND_CENTRES, S.BAND_AMPLITUDES):
        occupied = 1.35 / sps
        assert abs(e.centre - fc) <= occupied / 4, (e, fc)
        assert 0.90 <= e.bandwidth / occupied <= 1.25, (e, occupied)
        assert abs(e.power_dbfs - 20 * np.log10(amp)) <= 1.0, (e, amp)
        assert e.snr_db > 6.0
        shift, L, D, fill = frontend.channel_plan(e.centre, e.bandwidth)
        assert shift == -e.centre and 1 <= L <= _cabi.RESAMPLE_MAX_INTERPOLATE and 1 <= D <= _cabi.RESAMPLE_MAX_DECIMATE
        assert 8 / 1.25 <= sps * L / D <= 8 / 0.90, (sps, L, D)
        assert abs(fill - e.bandwidth * D / L) < 1e-12 and abs(fill / frontend.DEFAULT_FILL - 1) <= 0.0101


def test_noise_alone_and_a_lone_dc_spike_give_nothing():
    nfft = 1024
    w = frontend.design_window(nfft)
    k = frontend.window_scale(w)
    noise = S.band_psd(S.synthetic_band(5, pairs=1 << 17, emitters=False, dc=False), nfft, w, k)
    assert frontend.find_emitters(noise, window=w) == []
    spike = S.band_psd(S.synthetic_band(5, pairs=1 << 17, emitters=False), nfft, w, k)
    assert spike[0] > 1000 * np.median(spike)                                             # the DC offset towers over the floor
    assert frontend.find_emitters(spike, window=w) == []
    (dc,) = frontend.find_emitters(spike, window=w, dc_guard=-1, min_bins=1)              # without the guard it is an "emitter" at 0
    assert abs(dc.centre) < 1.0 / nfft and dc.bandwidth == 3.0 / nfft


def test_find_emitters_rules_on_a_hand_made_spectrum():
    p = np.ones(64)
    p[[1, 2, 3]] = 100.0                       # a run of three
    p[[8, 9, 12, 13]] = 100.0                  # two runs of two, two bins apart: joined into one of six
    p[[18, 19, 23, 24]] = 100.0                # three bins apart: not joined, each too short
    p[30] = 50.0                               # a single bin
    found = frontend.find_emitters(p, dc_guard=0)
    f = np.fft.fftfreq(64)
    assert [round(e.bandwidth * 64) for e in found] == [3, 6] and found[0].centre < found[1].centre      # both at positive frequencies, in order of centre
    by_width = {round(e.bandwidth * 64): e for e in found}
    assert abs(by_width[3].centre - f[2]) < 1e-12 and abs(by_width[6].centre - (f[8] + f[9] + f[12] + f[13]) / 4) < 1e-12
    assert abs(by_width[3].power_dbfs - 10 * np.log10(3 * 99.0)) < 1e-9 and abs(by_width[3].snr_db - 20.0) < 1e-9
    assert [round(e.bandwidth * 64) for e in frontend.find_emitters(p, dc_guard=0, merge_bins=3)] == [3, 6, 7]      # 18..24 now join
    wrap = np.ones(64)
    wrap[[30, 31, 32, 33]] = 100.0             # natural bins 30, 31 are +0.47, +0.48; 32, 33 are -0.5, -0.48: one signal across the edge
    two = frontend.find_emitters(wrap, min_bins=2)
    assert len(two) == 2 and two[0].centre < -0.48 and two[1].centre > 0.46
    with pytest.raises(ValueError):
        frontend.channel_plan(0.1, 1e-6)                                                     # would want a decimation far beyond 256
    with pytest.raises(ValueError):
        frontend.channel_plan(0.7, 0.01)


def test_plan_taps_exist_for_every_plan_the_limits_allow():
    """scan_iq's filters: the default design where 1024 taps hold it, the same design cut to 1024 taps beyond (max(L, D) > 128)."""
    np.testing.assert_array_equal(frontend.plan_taps(1, 1), np.array([32767], np.int16))
    np.testing.assert_array_equal(frontend.plan_taps(1, 12), frontend.design_lowpass(12))
    np.testing.assert_array_equal(frontend.plan_taps(5, 6), frontend.design_resampler(5, 6))
    for L, D in ((1, 256), (1, 129), (26, 145), (24, 143), (32, 255), (31, 256), (5, 54), (7, 18), (32, 1)):
        h = frontend.plan_taps(L, D)
        assert h.dtype == np.int16 and h.size == min(8 * max(L, D), _cabi.RESAMPLE_MAX_TAPS)
        for r in range(L):
            assert int(h[r::L].astype(np.int64).sum()) == 32768 and int(np.abs(h[r::L].astype(np.int64)).sum()) <= _cabi.RESAMPLE_MAX_BRANCH_ABS_SUM
