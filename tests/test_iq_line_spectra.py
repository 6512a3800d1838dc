"""mdc_iq_line_spectra / mdc_iq_line_spectra_rows / mdc_iq_find_lines and detect_iq(refine=True)'s rule, without a GPU:

  1. every argument error is MDC_EINVAL (-22) with a message, before any device call;
  2. mdc_iq_line_spectra_rows against tests/iq_spectrum_ref.rows_count, job by job;
  3. frontend.find_line after the refactoring against a literal restatement of what it was, on random spectra;
  4. the refinement rule -- isolate, find the lines, make the plan -- on the float64 reference spectra of the hopper
     (tests/iq_components_ref.hopping_band(1), boxes found with dc_guard = 0).  The bars come from a float64 run of this chain over
     seeds 1, 2, 3 (21 dwells, QPSK at 32 samples per symbol): symbol-rate error at most 2.0e-4 relative, bar 1e-3; carrier error
     at most 1.2e-6 cycles per sample (x^4 line 16.3 - 18.3 dB; the x^2 line, 1.8 - 3.2 dB, is rejected), bar 1e-5; the plan
     exactly 1/4.  This holds the recipe, not the kernels: those are tests/test_iq_line_spectra_gpu.py's."""
import ctypes
import functools

import numpy as np
import pytest

import iq_components_ref as CR
import iq_ddc_ref as D
import iq_line_ref as R
import iq_spectrum_ref as S
from modulationdetectioncnn_amd import _cabi, capture, frontend

JOB, BAND = _cabi.IQ_LINE_JOB, _cabi.IQ_LINE_BAND
EINVAL = -22


def _lib():
    L = _cabi.lib()
    L.mdc_last_error.restype = ctypes.c_char_p
    return L


def _jobs(spans, pairs_in, nfft, hop, avg):
    rec = np.zeros(len(spans), JOB)
    for k, (first, pairs) in enumerate(spans):
        rec[k] = (first, pairs, 0, 0)
    total = _lib().mdc_iq_line_spectra_rows(rec.ctypes.data, rec.size, pairs_in, nfft, hop, avg)
    return rec, total


# ------------------------------------------------------------------------------------------------------------ 1. validation
def test_line_spectra_rejects_bad_arguments_before_any_device_call():
    L = _lib()
    nfft, hop, avg, pairs_in = 64, 32, 2, 1000
    rec, total = _jobs([(0, 500), (100, 0), (300, 700)], pairs_in, nfft, hop, avg)
    assert total == int(rec["rows"].sum()) > 0
    buf = (ctypes.c_uint8 * 4096)()      # host memory stands in for device buffers: every check comes before a launch
    a = ctypes.addressof(buf)
    a += -a % 16
    orders = (ctypes.c_int * 4)(0, 2, 4, 1)

    def call(iq=a, fmt=2, pin=pairs_in, jh=rec.ctypes.data, jd=a, nj=rec.size, o=orders, no=3, n=nfft, h=hop, v=avg, w=a, scale=1.0, rows=a, tot=total,
             mean=a):
        return L.mdc_iq_line_spectra(iq, fmt, pin, jh, jd, nj, o, no, n, h, v, w, scale, rows, tot, mean, None)

    def refused(word, **kw):
        assert call(**kw) == EINVAL and word in L.mdc_last_error(), (kw, L.mdc_last_error())

    refused(b"null jobs", jh=None)
    refused(b"null orders", o=None)
    refused(b"null buffer", jd=None)
    refused(b"null buffer", mean=None)
    refused(b"null buffer", iq=None)
    refused(b"null buffer", w=None)
    refused(b"null buffer", rows=None)
    refused(b"unknown sample format", fmt=3)
    refused(b"order 1 must be", o=(ctypes.c_int * 3)(0, 3, 4))
    refused(b"appears twice", o=(ctypes.c_int * 3)(4, 2, 4))
    refused(b"norders", no=0)
    refused(b"norders", no=5)
    refused(b"nfft", n=96)
    refused(b"nfft", n=8192)
    refused(b"hop", h=0)
    refused(b"avg", v=0)
    refused(b"scale", scale=0.0)
    refused(b"scale", scale=float("inf"))
    refused(b"total_rows is", tot=total + 1)
    refused(b"total_rows is", tot=0)
    refused(b"mean_dev must be 8-byte aligned", mean=a + 4)
    refused(b"rows_dev must be 4-byte aligned", rows=a + 2)
    refused(b"window_dev must be 2-byte aligned", w=a + 1)
    refused(b"whole (I,Q) pair", iq=a + 2)
    outside = rec.copy()
    outside["pairs"][2] = 701
    refused(b"job 2: the stretch [300, 300 + 701)", jh=outside.ctypes.data)
    negative = rec.copy()
    negative["first_pair"][1] = -1
    refused(b"job 1:", jh=negative.ctypes.data)
    stale = rec.copy()
    stale["first_row"][2] += 1      # a table the rows function did not fill
    refused(b"job 2: first_row / rows", jh=stale.ctypes.data)
    # the rows function refuses the same jobs, and bad shapes, with a negative count
    assert L.mdc_iq_line_spectra_rows(outside.ctypes.data, 3, pairs_in, nfft, hop, avg) == EINVAL and b"job 2" in L.mdc_last_error()
    assert L.mdc_iq_line_spectra_rows(rec.ctypes.data, 3, pairs_in, 100, hop, avg) == EINVAL and b"nfft" in L.mdc_last_error()
    assert L.mdc_iq_line_spectra_rows(None, 1, pairs_in, nfft, hop, avg) == EINVAL and b"null jobs" in L.mdc_last_error()
    assert L.mdc_iq_line_spectra_rows(rec.ctypes.data, -1, pairs_in, nfft, hop, avg) == EINVAL
    # nothing to do: no jobs is MDC_OK without a launch, whatever the buffers
    assert L.mdc_iq_line_spectra_rows(None, 0, pairs_in, nfft, hop, avg) == 0
    assert call(jh=None, jd=None, nj=0, tot=0, iq=None, w=None, rows=None, mean=None) == 0


def test_find_lines_rejects_bad_arguments_before_any_device_call():
    L = _lib()
    buf = (ctypes.c_uint8 * 256)()
    a = ctypes.addressof(buf)
    a += -a % 16
    bands = np.zeros(3, BAND)
    bands[:] = [(0.1, 0.2, 0, 0), (0.0, 0.3, 1, 0), (0.25, 0.25, 0, 0)]

    def call(sp=a, n=3, nfft=64, bh=bands.ctypes.data, bd=a, rec=a):
        return L.mdc_iq_find_lines(sp, n, nfft, bh, bd, rec, None)

    def refused(word, **kw):
        assert call(**kw) == EINVAL and word in L.mdc_last_error(), (kw, L.mdc_last_error())

    refused(b"nfft", nfft=32)
    refused(b"nfft", nfft=192)
    refused(b"nfft", nfft=8192)
    refused(b"nspectra", n=-1)
    refused(b"null bands", bh=None)
    refused(b"null buffer", sp=None)
    refused(b"null buffer", bd=None)
    refused(b"null buffer", rec=None)
    refused(b"8-byte aligned", sp=a + 4)
    refused(b"8-byte aligned", rec=a + 4)
    for lo, hi, two in ((0.2, 0.1, 0), (0.501, 0.6, 0), (0.1001 / 6.4, 0.1002 / 6.4, 0), (float("nan"), 0.2, 0), (-0.2, -0.1, 1)):
        empty = bands.copy()
        empty[1] = (lo, hi, two, 0)
        refused(b"spectrum 1: no bin", bh=empty.ctypes.data)
    reserved = bands.copy()
    reserved["reserved"][2] = 1
    refused(b"spectrum 2: reserved", bh=reserved.ctypes.data)
    assert call(n=0, sp=None, bh=None, bd=None, rec=None) == 0


# ------------------------------------------------------------------------------------------------------------ 2. rows
@pytest.mark.parametrize("nfft,hop,avg", [(64, 32, 3), (64, 67, 2), (64, 1, 1), (1024, 512, 8), (4096, 4099, 2)])
def test_rows_function_is_the_reference_count_job_by_job(nfft, hop, avg):
    rng = np.random.default_rng(nfft + hop)
    pairs_in = nfft + 40 * avg * hop
    spans = [(0, 0), (3, nfft - 1), (5, nfft), (7, nfft + (avg - 1) * hop), (1, nfft + (3 * avg - 1) * hop + hop - 1),
             (pairs_in - nfft, nfft), (0, pairs_in), (pairs_in, 0)]
    spans += [(int(a), int(rng.integers(0, pairs_in - a + 1))) for a in rng.integers(0, pairs_in + 1, size=20)]
    rec, total = _jobs(spans, pairs_in, nfft, hop, avg)
    want = [S.rows_count(p, nfft, hop, avg) for _, p in spans]
    assert rec["rows"].tolist() == want and total == sum(want)
    assert rec["first_row"].tolist() == np.concatenate([[0], np.cumsum(want)[:-1]]).tolist()
    assert want[0] == 0 and want[1] == 0 and want[2] == (1 if avg == 1 else 0) and want[3] == 1 and want[4] == 3
    assert [(int(j["first_pair"]), int(j["pairs"])) for j in rec] == spans      # the stretches are left as given


# ------------------------------------------------------------------------------------------------------------ 3. find_line
def _find_line_literal(psd, lo, hi, two_sided=False):
    """frontend.find_line as it stood before its arithmetic moved into a helper"""
    p = np.array(psd, dtype=np.float64).reshape(-1)
    n = p.size
    f = np.fft.fftfreq(n)
    g = np.abs(f) if two_sided else f
    band = np.flatnonzero((g >= lo) & (g <= hi))
    k = int(band[np.argmax(p[band])])
    peak, floor = float(p[k]), float(np.median(p[band]))
    prominence = 10.0 * np.log10(peak / floor) if floor > 0.0 and peak > 0.0 else (np.inf if peak > 0.0 else 0.0)
    left, right = float(p[(k - 1) % n]), float(p[(k + 1) % n])
    delta = 0.0
    if left > 0.0 and peak > 0.0 and right > 0.0:
        a, b, c = np.log(left), np.log(peak), np.log(right)
        den = a - 2.0 * b + c
        if den < 0.0:
            delta = 0.5 * (a - c) / den
    return float(f[k] + delta / n), float(prominence)


def test_find_line_is_unchanged_by_the_refactoring():
    rng = np.random.default_rng(11)
    for n in (64, 100, 1024, 4096):
        for trial in range(40):
            p = rng.exponential(size=n)
            if trial % 4 == 1:
                p[rng.integers(0, n)] *= 50.0
            if trial % 4 == 2:
                p[rng.integers(0, n, size=n // 2)] = 0.0      # a zero median, zero neighbours
            if trial % 4 == 3:
                p[:] = np.round(p * 2.0) / 2.0                # ties
            lo = float(rng.uniform(0.0, 0.3))
            hi = lo + float(rng.uniform(2.0 / n, 0.2))
            for band in ((lo, hi, False), (-hi, -lo, False), (lo, hi, True), (0.0, hi, True), (-0.5, 0.5, False)):
                assert frontend.find_line(p, *band) == _find_line_literal(p, *band), (n, trial, band)
    assert frontend.find_line(np.zeros(64), 0.1, 0.2) == _find_line_literal(np.zeros(64), 0.1, 0.2) == (0.109375, 0.0)


# ------------------------------------------------------------------------------------------------------------ 4. the rule
@functools.lru_cache(maxsize=None)
def _hopper():
    iq, truth = CR.hopping_band(1)
    w = frontend.design_window(CR.HOP_NFFT)
    P = S.spectrogram(iq, "ci16", CR.HOP_NFFT, CR.HOP_NFFT // 2, CR.HOP_AVG, w, frontend.window_scale(w))[0].astype(np.float32)
    thresh = CR.detection_threshold(P, dc_guard=0)
    _, records, count = CR.components(P, thresh, 2, 3)
    found = frontend.detections_from_components(P, thresh, records.view(_cabi.IQ_COMPONENT), count, avg=CR.HOP_AVG)
    return iq, truth, found


def _mean_in_row_order(rows):
    acc = np.zeros(rows.shape[1], np.float64)
    for r in range(rows.shape[0]):
        acc += rows[r].astype(np.float64)
    return acc / float(rows.shape[0])


def test_refinement_rule_on_the_reference_spectra_of_the_hopper():
    iq, truth, found = _hopper()
    assert len(found) == len(truth) == 7
    nfft, avg = 1024, 8
    w = frontend.design_window(nfft)
    scale = frontend.window_scale(w)
    for d, (first, stop, centre, _) in zip(found, truth):
        plan = frontend.channel_plan(d.centre, d.bandwidth)[:3]
        assert plan[1:] in ((14, 59), (25, 108))                       # the width's guess: 7.59 or 7.41 samples per symbol
        D0, bands = capture._line_bands(d.bandwidth, nfft)
        assert D0 == min(max(int(1.0 / (4.0 * d.bandwidth)), 1), 256) and bands is not None
        part = iq[2 * d.first_pair:2 * d.stop_pair]
        iso = D.ddc(part, "ci16", 0, frontend.phase_step(-d.centre), D0, frontend.plan_taps(1, D0)).reshape(-1)
        lines = []
        for order, band in zip((0, 2, 4), bands):
            rows = R.line_spectrum(iso, "ci16", order, nfft, nfft // 2, avg, w, scale)[0]
            assert rows.shape[0] >= 1
            lines.append(frontend.find_line(_mean_in_row_order(rows), *band))
        (shift, L, Dn), extra = capture._refined_plan(d.centre, D0, plan, lines, 8.0)
        assert (L, Dn) == (1, 4)
        assert extra["symbol_rate"] is not None and abs(extra["symbol_rate"] * CR.HOP_SPS - 1.0) <= 1e-3, extra
        assert extra["symbol_line_db"] >= 8.0 and extra["symbol_line_db"] == lines[0][1]
        assert extra["carrier_order"] == 4 and lines[1][1] < 8.0 <= extra["carrier_line_db"] == lines[2][1]
        assert abs(d.centre + extra["carrier_offset"] - centre) <= 1e-5, (d.centre, extra, centre)
        folded = -(d.centre + extra["carrier_offset"])
        assert shift == (folded - round(folded) if abs(folded) > 0.5 else folded) and abs(shift) <= 0.5
        # a bar the lines do not reach: the plan stands, the centroid stands, the prominences are still reported
        kept, none = capture._refined_plan(d.centre, D0, plan, lines, 99.0)
        assert kept[1:] == plan[1:] and none["symbol_rate"] is None and none["carrier_order"] == 0 and none["carrier_offset"] == 0.0
        assert none["symbol_line_db"] == lines[0][1] and none["carrier_line_db"] == max(lines[1][1], lines[2][1])
    # no spectrum at all (too short for a row, or no bin in the band): the plan, and the five keys say so
    plan = (-0.1, 5, 6)
    kept, none = capture._refined_plan(0.1, 3, plan, None, 8.0)
    assert kept == plan and none == dict(symbol_rate=None, symbol_line_db=float("-inf"), carrier_offset=0.0, carrier_order=0,
                                         carrier_line_db=float("-inf"))
    assert capture._line_bands(1e-5, 64) == (256, None)      # b = 0.00256: the band 0.001 .. 0.0032 lies below the first bin of 64
