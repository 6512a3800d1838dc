"""mdc_iq_line_spectrum / frontend.line_spectrum / the estimators / VTCNN2.scan_iq(refine=True) on the MI355X, against
tests/iq_line_ref.py (float64 numpy, written from include/mdc.h):

  1. parity: orders 0, 2, 4 x the three formats x nfft in {64, 128, 256, 4096} (fewer butterflies than lanes with an even and an
     odd log2, one butterfly per thread, two per thread) x (hop, avg) in {(1, 1), (nfft/2, 3), (nfft+3, 2)}, on a capture just long
     enough for 5 rows, on pairs == nfft and on pairs == nfft - 1; the base pointer one pair into a larger allocation; the output
     pre-filled with a sentinel, one guard row after it untouched; the capture recipe of the spectrogram's test: uniform over the
     full range with planted runs of all-minimum (the 2^31 / 2^62 corner), all-maximum and alternating pairs, the later part two
     off-bin tones 40 dB apart (the first at +0.1235: its square at +0.2469, its fourth power at +0.4938, just below the fold --
     a conjugated staging puts them at -0.2469 and -0.4938); design_window and an asymmetric random window.  The tolerance is the
     header's, every term from the reference:
         |P^ - P| <= mean_s[2 eps sqrt(P_s[k] T_s) + eps^2 T_s] + (avg + 4) u P[r,k],  u = 2^-24, eps = u (8 (log2 nfft + 1) + 2);
  2. order 1 is mdc_iq_spectrogram, bit for bit;
  3. the same call twice gives the same bits; row r of a 9-row call is, bit for bit, the one row of the sub-capture from r avg hop;
  4. past the grid cap: picked rows against the reference, the whole output against a two-piece run split off the cap's grid;
  5. frontend.line_spectrum replays bit-identically from a captured graph after the input is overwritten;
  6. VTCNN2.scan_iq(refine=True) end to end: the plans, the estimates, and its results against isolating, estimating, resampling
     and classifying by hand; refine=False is the call without the argument;
  7. the example's --scan --refine path."""
import functools
import importlib.util
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import iq_line_ref as R                                                                  # noqa: E402
import iq_spectrum_ref as S                                                              # noqa: E402
from conftest import GOLDEN, ROOT                                                        # noqa: E402
from modulationdetectioncnn_amd import VTCNN2, _cabi, frontend                           # noqa: E402

FORMATS = ["cu8", "ci8", "ci16"]
ORDERS = [0, 2, 4]
SENTINEL = -7.0


def _capture(fmt, pairs, seed):
    """One pair of padding + `pairs` pairs + one pair of padding.  Uniform over the whole range; from the middle on two off-bin
    tones, 0.6 and 0.006 of full scale; runs of 300 pairs of all minimum, all maximum and alternating minimum / maximum pairs at
    pairs 0, 700, 1500 and 200 before the end (cut off where the capture is shorter)."""
    lo, hi, dt = S.SAMPLE_MIN[fmt], S.SAMPLE_MAX[fmt], S.DTYPE[fmt]
    rng = np.random.default_rng(seed)
    buf = rng.integers(lo, hi + 1, size=2 * (pairs + 2)).astype(dt)
    body = buf[2:2 + 2 * pairs]
    half = pairs // 2
    n = np.arange(half, pairs)
    z = 0.6 * np.exp(2j * np.pi * (0.1234567 * n + 0.3)) + 0.006 * np.exp(-2j * np.pi * (0.3141593 * n + 0.1))
    mid, amp = (lo + hi) / 2.0, (hi - lo) / 2.0
    body[2 * half:] = np.clip(np.rint(np.stack([z.real, z.imag], axis=1) * amp + mid), lo, hi).astype(dt).reshape(-1)
    alt = np.empty(600, dt)
    alt[0::4], alt[1::4], alt[2::4], alt[3::4] = lo, lo, hi, hi
    for at, run in ((0, np.full(600, lo, dt)), (700, np.full(600, hi, dt)), (1500, alt), (max(0, pairs - 200), np.full(600, lo, dt))):
        seg = body[2 * at: 2 * at + 600]
        seg[:] = run[:seg.size]
    return buf


def _random_window(nfft, seed):
    return np.random.default_rng(seed).integers(0, 32768, size=nfft).astype(np.int16)      # asymmetric: a reversed or shifted index shows


def _line(dev, fmt, pairs, order, nfft, hop, avg, wdev, scale):
    """mdc_iq_line_spectrum straight through the binding; dev: the device tensor whose data_ptr is pair 0.  Returns the
    (rows, nfft) device tensor after checking the guard row."""
    L = _cabi.lib()
    rows = L.mdc_iq_spectrogram_rows(pairs, nfft, hop, avg)
    assert rows == S.rows_count(pairs, nfft, hop, avg)
    out = torch.full((rows + 1, nfft), SENTINEL, dtype=torch.float32, device="cuda")
    _cabi.check(L.mdc_iq_line_spectrum(dev.data_ptr(), S.FMT[fmt], pairs, order, nfft, hop, avg, wdev.data_ptr(), scale, out.data_ptr(), rows,
                                       torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert bool((out[rows] == SENTINEL).all())
    return out[:rows]


def _worst_ratio(got, iq, fmt, order, nfft, hop, avg, w, scale, rows=None):
    """largest |got - P| / bound over the rows (all, or the listed ones), every term of the bound from the float64 reference"""
    P, Ps, Ts = R.line_spectrum(iq, fmt, order, nfft, hop, avg, w, scale, rows)
    assert got.shape == P.shape
    if P.size == 0:
        return 0.0
    assert np.all(np.isfinite(got)) and got.min() >= 0.0                                   # in particular no sentinel is left
    return float((np.abs(got.astype(np.float64) - P) / R.bound(P, Ps, Ts, nfft, avg, order)).max())


# ---------------------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("nfft", [64, 128, 256, 4096])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("order", ORDERS)
def test_line_spectrum_is_the_reference(order, fmt, nfft):
    worst = 0.0
    windows = [frontend.design_window(nfft), _random_window(nfft, seed=nfft)]
    for hop, avg in ((1, 1), (nfft // 2, 3), (nfft + 3, 2)):
        for pairs in (nfft + (5 * avg - 1) * hop, nfft, nfft - 1):
            buf = _capture(fmt, pairs, seed=nfft + hop + pairs)
            dev = torch.from_numpy(buf).cuda()[2:]                   # one pair into the allocation
            assert dev.data_ptr() % 256 == _cabi.IQ_PAIR_BYTES[S.FMT[fmt]]
            for w in windows:
                scale = frontend.window_scale(w)
                got = _line(dev, fmt, pairs, order, nfft, hop, avg, torch.from_numpy(w).cuda(), scale).cpu().numpy()
                assert got.shape == (5 if pairs > nfft else 1 if pairs == nfft and avg == 1 else 0, nfft)
                ratio = _worst_ratio(got, buf[2:2 + 2 * pairs], fmt, order, nfft, hop, avg, w, scale)
                worst = max(worst, ratio)
                assert ratio <= 1.0, (order, fmt, nfft, hop, avg, pairs, ratio)
    print(f"order {order} {fmt} nfft {nfft}: largest error / bound {worst:.4f}")


# ---------------------------------------------------------------------------------------------------------------- 2. order 1
@pytest.mark.parametrize("nfft", [128, 4096])
@pytest.mark.parametrize("fmt", FORMATS)
def test_order_one_is_the_spectrogram_bit_for_bit(fmt, nfft):
    L = _cabi.lib()
    hop, avg = nfft // 2 + 1, 3
    pairs = nfft + (5 * avg - 1) * hop
    buf = _capture(fmt, pairs, seed=nfft + 1)
    dev = torch.from_numpy(buf).cuda()[2:]
    for w in (frontend.design_window(nfft), _random_window(nfft, seed=5)):
        wdev, scale = torch.from_numpy(w).cuda(), frontend.window_scale(w)
        line = _line(dev, fmt, pairs, 1, nfft, hop, avg, wdev, scale)
        spec = torch.full((5, nfft), SENTINEL, dtype=torch.float32, device="cuda")
        _cabi.check(L.mdc_iq_spectrogram(dev.data_ptr(), S.FMT[fmt], pairs, nfft, hop, avg, wdev.data_ptr(), scale, spec.data_ptr(), 5,
                                         torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert line.shape == spec.shape and torch.equal(line.view(torch.int32), spec.view(torch.int32))
        assert float(spec.min()) >= 0.0
    body = torch.from_numpy(buf[2:2 + 2 * pairs].copy()).cuda()
    assert torch.equal(frontend.line_spectrum(body, fmt, 1, nfft=nfft, avg=avg), frontend.spectrogram(body, fmt, nfft=nfft, avg=avg))


# ---------------------------------------------------------------------------------------------------------------- 3. determinism, seams
@pytest.mark.parametrize("nfft", [256, 4096])
def test_determinism_and_seam_identity(nfft):
    fmt, order, hop, avg, rows = "ci16", 4, nfft // 2 + 1, 3, 9
    pairs = nfft + (rows * avg - 1) * hop
    buf = _capture(fmt, pairs, seed=nfft)
    dev = torch.from_numpy(buf).cuda()[2:]
    w = _random_window(nfft, seed=3)
    wdev, scale = torch.from_numpy(w).cuda(), frontend.window_scale(w)
    whole = _line(dev, fmt, pairs, order, nfft, hop, avg, wdev, scale)
    assert whole.shape == (rows, nfft)
    assert torch.equal(whole, _line(dev, fmt, pairs, order, nfft, hop, avg, wdev, scale))
    assert _worst_ratio(whole.cpu().numpy(), buf[2:2 + 2 * pairs], fmt, order, nfft, hop, avg, w, scale) <= 1.0
    one = nfft + (avg - 1) * hop                                 # pairs of exactly one row
    for r in range(rows):
        piece = _line(dev[2 * r * avg * hop:], fmt, one, order, nfft, hop, avg, wdev, scale)
        assert piece.shape == (1, nfft) and torch.equal(piece[0], whole[r]), (nfft, r)


# ---------------------------------------------------------------------------------------------------------------- 4. past the grid cap
def test_stride_loop_past_the_grid_cap():
    nfft, hop, avg, fmt, order = 64, 64, 1, "ci16", 2
    cap = _cabi.SPECTROGRAM_GRID_CAP
    rows = 2 * cap + 5
    pairs = nfft + (rows - 1) * hop
    g = torch.Generator(device="cuda").manual_seed(4)
    dev = torch.randint(-32768, 32768, (2 * pairs,), dtype=torch.int16, device="cuda", generator=g)
    iq = dev.cpu().numpy()
    w = _random_window(nfft, seed=9)
    wdev, scale = torch.from_numpy(w).cuda(), frontend.window_scale(w)
    whole = _line(dev, fmt, pairs, order, nfft, hop, avg, wdev, scale)
    assert whole.shape == (rows, nfft)
    rng = np.random.default_rng(8)
    picks = np.unique(np.concatenate([[0, rows - 1, cap - 1, cap, 2 * cap - 1, 2 * cap], rng.integers(0, rows, size=200)]))
    ratio = _worst_ratio(whole[torch.from_numpy(picks).cuda()].cpu().numpy(), iq, fmt, order, nfft, hop, avg, w, scale, rows=picks)
    print(f"largest error / bound {ratio:.4f}")
    assert ratio <= 1.0
    a = cap // 2 + 123                                           # rows of the first piece: the second piece's grid starts off the cap's
    first = _line(dev, fmt, a * hop, order, nfft, hop, avg, wdev, scale)
    second = _line(dev[2 * a * hop:], fmt, pairs - a * hop, order, nfft, hop, avg, wdev, scale)
    assert first.shape[0] == a and torch.equal(torch.cat([first, second]), whole)


# ---------------------------------------------------------------------------------------------------------------- 5. graph capture
def test_line_spectrum_is_capturable():
    nfft, avg, fmt, order = 1024, 2, "ci16", 4
    pairs = nfft + 11 * (nfft // 2)
    dev = torch.from_numpy(_capture(fmt, pairs, seed=1)[2:-2].copy()).cuda()
    frontend.line_spectrum(dev, fmt, order, nfft=nfft, avg=avg)      # warm: the cached window, code objects
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        p1 = frontend.line_spectrum(dev, fmt, order, nfft=nfft, avg=avg)
    assert p1.shape == (6, nfft)
    for seed in (2, 3):
        dev.copy_(torch.from_numpy(_capture(fmt, pairs, seed=seed)[2:-2].copy()).cuda())      # same buffer, new capture
        p1.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        pe = frontend.line_spectrum(dev, fmt, order, nfft=nfft, avg=avg)
        torch.cuda.synchronize()
        assert torch.equal(p1, pe) and float(pe.min()) >= 0.0, seed


# ---------------------------------------------------------------------------------------------------------------- 6. end to end
@functools.lru_cache(maxsize=None)
def _band():
    return S.synthetic_band(1)                                   # shared: nobody writes to it


def test_estimators_short_capture_and_thresholds():
    """a capture too short for one row is no error; a threshold above the line's prominence turns the estimate off"""
    short = torch.zeros(2 * 1000, dtype=torch.int16, device="cuda")
    assert frontend.estimate_symbol_rate(short, "ci16", 0.05, 0.3) == (None, float("-inf"))
    assert frontend.estimate_carrier_offset(short, "ci16", 0.03) == (0.0, 0, float("-inf"))
    dev = torch.from_numpy(_band().copy()).cuda()
    iso = frontend.ddc(dev, "ci16", shift=-S.BAND_CENTRES[1], decimate=8, taps=frontend.plan_taps(1, 8)).reshape(-1)
    rate, db = frontend.estimate_symbol_rate(iso, "ci16", 0.08, 0.3)
    assert rate is not None and abs(rate * S.BAND_SPS[1] / 8 - 1.0) <= 1e-3 and db >= 14.0
    assert frontend.estimate_symbol_rate(iso, "ci16", 0.08, 0.3, min_line_db=db + 1.0) == (None, db)
    offset, order, odb = frontend.estimate_carrier_offset(iso, "ci16", 0.03)
    assert order == 4 and abs(offset) / 8 <= 5e-6 and odb >= 14.0
    assert frontend.estimate_carrier_offset(iso, "ci16", 0.03, min_line_db=odb + 1.0) == (0.0, 0, odb)


def test_scan_iq_refine_is_isolate_estimate_resample_and_predict_by_hand():
    nfft, avg, iq = 1024, 8, _band()
    m = VTCNN2.from_npz(os.path.join(GOLDEN, "weights", "3convmodrecnets_CNN2_0.5.npz"))
    dev = torch.from_numpy(iq.copy()).cuda()
    records = m.scan_iq(dev, "ci16", refine=True, squelch_dbfs=-60.0)
    w = frontend.design_window(nfft)
    emitters = frontend.find_emitters(frontend.spectrogram(dev, "ci16", nfft=nfft, avg=avg).to(torch.float64).mean(0).cpu(), window=w)
    assert len(records) == len(emitters) == 3
    for rec, e, fc, sps, want in zip(records, emitters, S.BAND_CENTRES, S.BAND_SPS, ((1, 12), (1, 6), (2, 5))):
        assert (rec["centre"], rec["bandwidth"], rec["power_dbfs"], rec["snr_db"]) == tuple(e)      # centre stays the centroid
        assert (rec["interpolate"], rec["decimate"]) == want
        assert abs(rec["symbol_rate"] * sps - 1.0) <= 1e-3
        assert rec["carrier_order"] == 4
        assert abs(rec["centre"] + rec["carrier_offset"] - fc) <= 5e-6
        print(f"sps {sps}: symbol rate x sps - 1 = {rec['symbol_rate'] * sps - 1.0:+.2e} ({rec['symbol_line_db']:.1f} dB), carrier error "
              f"{rec['centre'] + rec['carrier_offset'] - fc:+.2e} ({rec['carrier_line_db']:.1f} dB; centroid {rec['centre'] - fc:+.2e})")
        # by hand, with the documented rule
        D0 = min(max(int(1.0 / (4.0 * e.bandwidth)), 1), 256)
        iso = frontend.ddc(dev, "ci16", shift=-e.centre, decimate=D0, taps=frontend.plan_taps(1, D0)).reshape(-1)
        b = e.bandwidth * D0
        rate, rate_db = frontend.estimate_symbol_rate(iso, "ci16", lo=b / 2.5, hi=min(0.45, 1.25 * b))
        offset, order, offset_db = frontend.estimate_carrier_offset(iso, "ci16", max_offset=b / 8.0)
        assert (rec["symbol_rate"], rec["symbol_line_db"]) == (rate / D0, rate_db)
        assert (rec["carrier_offset"], rec["carrier_order"], rec["carrier_line_db"]) == (offset / D0, order, offset_db)
        assert rate_db >= 14.0 and offset_db >= 14.0                 # 6 dB above the threshold
        L, D, _ = frontend.resample_ratio(1.0, rate / D0, 8)
        assert (L, D) == want and rec["shift"] == -(e.centre + offset / D0)
        taps = frontend.plan_taps(L, D)
        down = frontend.ddc(dev, "ci16", shift=rec["shift"], decimate=D, taps=taps) if L == 1 else \
            frontend.resample(dev, "ci16", shift=rec["shift"], interpolate=L, decimate=D, taps=taps)
        down = down[:down.shape[0] // 128 * 128]
        assert down.shape[0] >= 128
        p, l, d = m.predict_iq(down.reshape(-1), "ci16", normalize="rms", squelch_dbfs=-60.0, return_power=True)
        assert torch.equal(rec["probs"], p) and torch.equal(rec["labels"], l) and torch.equal(rec["window_dbfs"], d)
        open_ = l[l >= 0]
        assert open_.numel() > 0 and rec["label"] == int(torch.bincount(open_).argmax())
    by_numpy = m.scan_iq(iq, "ci16", refine=True, squelch_dbfs=-60.0)                        # numpy in, numpy out
    for rec, ref in zip(by_numpy, records):
        assert isinstance(rec["probs"], np.ndarray) and rec["label"] == ref["label"]
        assert (rec["interpolate"], rec["decimate"], rec["symbol_rate"], rec["carrier_offset"]) == \
            (ref["interpolate"], ref["decimate"], ref["symbol_rate"], ref["carrier_offset"])
        np.testing.assert_array_equal(rec["probs"].view(np.uint32), ref["probs"].cpu().numpy().view(np.uint32))
        np.testing.assert_array_equal(rec["labels"], ref["labels"].cpu().numpy())
    # refine=False is today's call: the same keys, the same values
    plain = m.scan_iq(dev, "ci16", squelch_dbfs=-60.0)
    off = m.scan_iq(dev, "ci16", refine=False, squelch_dbfs=-60.0)
    assert len(plain) == len(off) == 3
    for a, b_ in zip(plain, off):
        assert list(a) == list(b_) and "symbol_rate" not in a and set(records[0]) - set(a) == \
            {"symbol_rate", "symbol_line_db", "carrier_offset", "carrier_order", "carrier_line_db"}
        for key in a:
            assert torch.equal(a[key], b_[key]) if isinstance(a[key], torch.Tensor) else a[key] == b_[key], key
    m._release()


# ---------------------------------------------------------------------------------------------------------------- 7. the example
def test_example_scan_refine_prints_symbol_rates(capsys):
    spec = importlib.util.spec_from_file_location("classify_capture", os.path.join(ROOT, "examples", "classify_capture.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    model = VTCNN2.synthetic("deployed3")
    found = ex.scan(model, ex.synthetic_band("ci16"), "ci16", rate=2.4e6, refine=True)
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(found) == 3 and lines[0].startswith("3 emitters (Hz)") and len(lines) == 2 + 3
    assert lines[1].split()[-3:] == ["symbol", "rate", "refined"]
    for line, fc, sps in zip(lines[2:], S.BAND_CENTRES, S.BAND_SPS):
        cols = line.split()
        assert len(cols) == 10
        assert abs(float(cols[8]) / (2.4e6 / sps) - 1.0) <= 1e-3
        assert abs(float(cols[9]) - fc * 2.4e6) <= 5e-6 * 2.4e6
    model._release()
