"""mdc_iq_line_spectra / mdc_iq_find_lines / frontend.line_spectra / find_lines / VTCNN2.detect_iq(refine=True) on the MI355X:

  1. rows: every job's rows of every plane are, bit for bit, what mdc_iq_line_spectrum writes for the job's slice -- the three
     formats x nfft in {64, 128, 256, 4096} (fewer butterflies than lanes with an even and an odd log2, one butterfly per thread,
     two per thread) x (hop, avg) in {(nfft/2, 3), (nfft+3, 2), (1, 1)}; orders (0, 2, 4) in one call, (1,) and (4, 0) in two more
     (the plane's index is not the order); jobs of 0 pairs, of nfft - 1 pairs, of exactly one row, of 3 rows plus trailing
     segments, two that overlap, one from an odd pair, one that ends on the capture's last pair; outputs pre-filled with a
     sentinel, a guard row at both ends untouched;
  2. means: bit for bit the sequential float64 numpy loop over those rows; jobs without rows read 0.0;
  3. isolation: every pair outside one job overwritten with the format's extremes, the job's rows and mean keep their bits;
  4. past the grid cap: 2,101 + rows in one plane, the whole output against single calls;
  5. determinism: the same call twice; the jobs reversed; a replay from a captured graph after the capture was overwritten;
  6. find_lines against frontend.find_line, exact, on noise, planted lines, ties, peaks on bins 0 and nfft - 1, zero medians, all
     zeros; one- and two-sided bands, a single bin, even and odd counts, all bins; a NaN gives count -1 for its spectrum alone;
  7. detect_iq(refine=True) end to end against the recipe done by hand with the public pieces; batched against the loop;
  8. the example's --detections --refine lines."""
import functools
import importlib.util
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import iq_spectrum_ref as S                                                              # noqa: E402
from conftest import ROOT                                                                # noqa: E402
from modulationdetectioncnn_amd import VTCNN2, _cabi, frontend                           # noqa: E402

FORMATS = ["cu8", "ci8", "ci16"]
SENTINEL, SENTINEL64 = -7.0, -11.0
FIVE = ("symbol_rate", "symbol_line_db", "carrier_offset", "carrier_order", "carrier_line_db")


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


def _single(dev, fmt, first, pairs, order, nfft, hop, avg, wdev, scale):
    """the oracle: mdc_iq_line_spectrum on the slice, (rows, nfft) float32 on the device"""
    L = _cabi.lib()
    rows = _cabi.check(L.mdc_iq_spectrogram_rows(pairs, nfft, hop, avg))
    out = torch.empty((rows, nfft), dtype=torch.float32, device="cuda")
    at = dev.data_ptr() + first * _cabi.IQ_PAIR_BYTES[S.FMT[fmt]]
    _cabi.check(L.mdc_iq_line_spectrum(at if pairs else None, S.FMT[fmt], pairs, order, nfft, hop, avg, wdev.data_ptr(), scale,
                                       out.data_ptr() if rows else None, rows, torch.cuda.current_stream().cuda_stream))
    return out


def _table(spans, pairs_in, nfft, hop, avg):
    rec = np.zeros(len(spans), _cabi.IQ_LINE_JOB)
    for k, (first, pairs) in enumerate(spans):
        rec[k] = (first, pairs, 0, 0)
    total = _cabi.check(_cabi.lib().mdc_iq_line_spectra_rows(rec.ctypes.data, rec.size, pairs_in, nfft, hop, avg))
    return rec, total


def _batched(dev, fmt, pairs_in, spans, orders, nfft, hop, avg, wdev, scale):
    """One mdc_iq_line_spectra call into sentinel-filled buffers with a guard row at both ends: (rows (norders, total, nfft)
    float32, means (K, norders, nfft) float64, the job table), on the host; the guards are checked here"""
    rec, total = _table(spans, pairs_in, nfft, hop, avg)
    K, no = rec.size, len(orders)
    big = torch.full((no * total + 2, nfft), SENTINEL, dtype=torch.float32, device="cuda")
    bigm = torch.full((K * no + 2, nfft), SENTINEL64, dtype=torch.float64, device="cuda")
    jobs_dev = torch.from_numpy(rec.view(np.int64).reshape(K, 4)).cuda()
    o = np.asarray(orders, np.int32)
    _cabi.check(_cabi.lib().mdc_iq_line_spectra(dev.data_ptr(), S.FMT[fmt], pairs_in, rec.ctypes.data, jobs_dev.data_ptr(), K, o.ctypes.data, no, nfft, hop,
                                                avg, wdev.data_ptr(), scale, big[1:].data_ptr(), total, bigm[1:].data_ptr(),
                                                torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    rows, means = big.cpu().numpy(), bigm.cpu().numpy()
    assert (rows[0] == SENTINEL).all() and (rows[-1] == SENTINEL).all() and (means[0] == SENTINEL64).all() and (means[-1] == SENTINEL64).all()
    return rows[1:-1].reshape(no, total, nfft), means[1:-1].reshape(K, no, nfft), rec


def _mean_in_row_order(rows):
    acc = np.zeros(rows.shape[1], np.float64)
    for r in range(rows.shape[0]):
        acc += rows[r].astype(np.float64)
    return acc / float(rows.shape[0]) if rows.shape[0] else acc


def _hold_to_single_calls(dev, fmt, pairs_in, spans, orders, nfft, hop, avg, wdev, scale, oracle):
    """tests 1 and 2 for one call; oracle: a dict (job, order) -> the single call's rows on the host, filled on demand"""
    rows, means, rec = _batched(dev, fmt, pairs_in, spans, orders, nfft, hop, avg, wdev, scale)
    for k, (first, pairs) in enumerate(spans):
        a, n = int(rec["first_row"][k]), int(rec["rows"][k])
        for i, order in enumerate(orders):
            if (k, order) not in oracle:
                oracle[k, order] = _single(dev, fmt, first, pairs, order, nfft, hop, avg, wdev, scale).cpu().numpy()
            want = oracle[k, order]
            assert want.shape == (n, nfft) and rows[i, a:a + n].view(np.int32).tobytes() == want.view(np.int32).tobytes(), (fmt, nfft, hop, avg, k, order)
            assert means[k, i].view(np.int64).tobytes() == _mean_in_row_order(want).view(np.int64).tobytes(), (fmt, nfft, hop, avg, k, order)
            if n == 0:
                assert not means[k, i].any()
    return rows, means, rec


def _spans(nfft, hop, avg):
    """the job list of test 1 and the capture's length"""
    one = nfft + (avg - 1) * hop                              # exactly one row
    three = nfft + (4 * avg - 2) * hop + hop - 1              # 3 rows, then avg - 1 segments and hop - 1 pairs that fill no row
    two = nfft + (2 * avg - 1) * hop
    pairs_in = 16 + three + nfft
    spans = [(0, 0), (3, nfft - 1), (4, one), (2, three), (10, two), (10 + nfft // 3, two), (7, one + min(3, hop - 1)), (pairs_in - one, one), (pairs_in, 0)]
    return spans, pairs_in


# ---------------------------------------------------------------------------------------------------------------- 1, 2. rows and means
@pytest.mark.parametrize("nfft", [64, 128, 256, 4096])
@pytest.mark.parametrize("fmt", FORMATS)
def test_rows_are_the_single_calls_and_means_the_numpy_loop(fmt, nfft):
    for hop, avg in ((nfft // 2, 3), (nfft + 3, 2), (1, 1)):
        spans, pairs_in = _spans(nfft, hop, avg)
        buf = _capture(fmt, pairs_in, seed=nfft + hop)
        dev = torch.from_numpy(buf).cuda()[2:]                   # one pair into the allocation
        w = _random_window(nfft, seed=5) if hop == 1 else frontend.design_window(nfft)
        wdev, scale = torch.from_numpy(w).cuda(), frontend.window_scale(w)
        oracle = {}
        _, _, rec = _hold_to_single_calls(dev, fmt, pairs_in, spans, (0, 2, 4), nfft, hop, avg, wdev, scale, oracle)
        assert rec["rows"].tolist() == [0, 0, 1, 3, 2, 2, 1, 1, 0]
        _hold_to_single_calls(dev, fmt, pairs_in, spans, (1,), nfft, hop, avg, wdev, scale, oracle)
        _hold_to_single_calls(dev, fmt, pairs_in, spans, (4, 0), nfft, hop, avg, wdev, scale, oracle)


def test_jobs_without_any_row_write_zero_means_and_no_rows():
    nfft, pairs_in = 64, 500
    dev = torch.from_numpy(_capture("ci16", pairs_in, seed=3)).cuda()[2:]
    w = frontend.design_window(nfft)
    rows, means, rec = _batched(dev, "ci16", pairs_in, [(0, 0), (17, nfft - 1), (pairs_in, 0)], (0, 2, 4), nfft, 32, 2, torch.from_numpy(w).cuda(),
                                frontend.window_scale(w))
    assert rows.shape == (3, 0, nfft) and means.shape == (3, 3, nfft) and not means.any() and not rec["rows"].any()


# ---------------------------------------------------------------------------------------------------------------- 3. isolation
@pytest.mark.parametrize("fmt", FORMATS)
def test_a_job_reads_no_pair_outside_itself(fmt):
    nfft, hop, avg = 128, 64, 3
    spans, pairs_in = _spans(nfft, hop, avg)
    buf = _capture(fmt, pairs_in, seed=41)
    w = frontend.design_window(nfft)
    wdev, scale = torch.from_numpy(w).cuda(), frontend.window_scale(w)
    rows, means, rec = _batched(torch.from_numpy(buf).cuda()[2:], fmt, pairs_in, spans, (0, 2, 4), nfft, hop, avg, wdev, scale)
    lo, hi = S.SAMPLE_MIN[fmt], S.SAMPLE_MAX[fmt]
    for k in (3, 6):                                             # the 3-row job from pair 2, the job from the odd pair 7
        first, pairs = spans[k]
        other = buf.copy()
        body = other[2:2 + 2 * pairs_in]
        body[:2 * first] = np.where(np.arange(2 * first) % 3 == 0, lo, hi)
        tail = body[2 * (first + pairs):]
        tail[:] = np.where(np.arange(tail.size) % 3 == 0, hi, lo)
        other[:2], other[-2:] = hi, lo
        rows2, means2, _ = _batched(torch.from_numpy(other).cuda()[2:], fmt, pairs_in, spans, (0, 2, 4), nfft, hop, avg, wdev, scale)
        a, n = int(rec["first_row"][k]), int(rec["rows"][k])
        assert n >= 1 and rows2[:, a:a + n].tobytes() == rows[:, a:a + n].tobytes() and means2[k].tobytes() == means[k].tobytes()
        assert rows2.tobytes() != rows.tobytes()                 # (the other jobs did see the change)


# ---------------------------------------------------------------------------------------------------------------- 4. the grid cap
def test_more_rows_than_the_grid_cap():
    nfft, hop, avg = 64, 1, 1
    long_ = nfft + 2100
    pairs_in = long_ + 40
    spans = [(5, nfft + 2), (11, long_), (pairs_in - nfft, nfft)]
    dev = torch.from_numpy(_capture("ci8", pairs_in, seed=9)).cuda()[2:]
    w = _random_window(nfft, seed=6)
    _, _, rec = _hold_to_single_calls(dev, "ci8", pairs_in, spans, (0, 2, 4), nfft, hop, avg, torch.from_numpy(w).cuda(), frontend.window_scale(w), {})
    assert rec["rows"].tolist() == [3, 2101, 1] and int(rec["rows"].sum()) > _cabi.SPECTROGRAM_GRID_CAP


# ---------------------------------------------------------------------------------------------------------------- 5. determinism
def test_determinism_job_order_and_graph_replay():
    fmt, nfft, hop, avg = "ci16", 256, 128, 3
    spans, pairs_in = _spans(nfft, hop, avg)
    buf = _capture(fmt, pairs_in, seed=17)
    dev = torch.from_numpy(buf).cuda()[2:]
    w = frontend.design_window(nfft)
    wdev, scale = torch.from_numpy(w).cuda(), frontend.window_scale(w)
    orders = (0, 2, 4)
    rows, means, rec = _batched(dev, fmt, pairs_in, spans, orders, nfft, hop, avg, wdev, scale)
    again = _batched(dev, fmt, pairs_in, spans, orders, nfft, hop, avg, wdev, scale)
    assert again[0].tobytes() == rows.tobytes() and again[1].tobytes() == means.tobytes()
    back = _batched(dev, fmt, pairs_in, spans[::-1], orders, nfft, hop, avg, wdev, scale)
    K = len(spans)
    for k in range(K):
        a, n = int(rec["first_row"][k]), int(rec["rows"][k])
        b = int(back[2]["first_row"][K - 1 - k])
        assert int(back[2]["rows"][K - 1 - k]) == n and back[0][:, b:b + n].tobytes() == rows[:, a:a + n].tobytes()
        assert back[1][K - 1 - k].tobytes() == means[k].tobytes()
    # the package entry gives the same bits, and its shapes
    m, counts, r, first = frontend.line_spectra(dev[:2 * pairs_in], fmt, [(a, a + p) for a, p in spans], orders, nfft=nfft, hop=hop, avg=avg, return_rows=True)
    assert m.dtype == torch.float64 and tuple(m.shape) == (K, 3, nfft) and r.dtype == torch.float32 and tuple(r.shape) == rows.shape
    assert counts.dtype == np.int64 and counts.tolist() == rec["rows"].tolist() and first.tolist() == rec["first_row"].tolist() + [int(rec["rows"].sum())]
    assert m.cpu().numpy().tobytes() == means.tobytes() and r.cpu().numpy().tobytes() == rows.tobytes()
    offsets = np.array([0, 700, 700, 1500, pairs_in], np.int64)      # K + 1 offsets, as extract returns them
    m2, c2 = frontend.line_spectra(dev[:2 * pairs_in], fmt, offsets, orders, nfft=nfft, hop=hop, avg=avg)
    m3, c3 = frontend.line_spectra(dev[:2 * pairs_in], fmt, list(zip(offsets[:-1], offsets[1:])), orders, nfft=nfft, hop=hop, avg=avg)
    assert tuple(m2.shape) == (4, 3, nfft) and c2.tolist() == c3.tolist() and c2[1] == 0 and torch.equal(m2, m3) and not m2[1].any()
    # a captured graph: the call allocates and copies nothing; replayed on a new capture in the same buffer
    total = int(rec["rows"].sum())
    jobs_dev = torch.from_numpy(rec.view(np.int64).reshape(K, 4)).cuda()
    out = torch.full((3, total, nfft), SENTINEL, dtype=torch.float32, device="cuda")
    outm = torch.full((K, 3, nfft), SENTINEL64, dtype=torch.float64, device="cuda")
    o = np.asarray(orders, np.int32)
    L = _cabi.lib()

    def call(stream):
        _cabi.check(L.mdc_iq_line_spectra(dev.data_ptr(), S.FMT[fmt], pairs_in, rec.ctypes.data, jobs_dev.data_ptr(), K, o.ctypes.data, 3, nfft, hop, avg,
                                          wdev.data_ptr(), scale, out.data_ptr(), total, outm.data_ptr(), stream.cuda_stream))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        call(side)
    torch.cuda.synchronize()
    other = _capture(fmt, pairs_in, seed=18)
    full = torch.from_numpy(other).cuda()
    want = _batched(full[2:], fmt, pairs_in, spans, orders, nfft, hop, avg, wdev, scale)
    dev.copy_(full[2:])                                          # overwritten ...
    out.fill_(SENTINEL)
    outm.fill_(SENTINEL64)
    g.replay()
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == want[0].tobytes() != rows.tobytes() and outm.cpu().numpy().tobytes() == want[1].tobytes()
    dev.copy_(torch.from_numpy(buf).cuda()[2:])                  # ... and restored
    g.replay()
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == rows.tobytes() and outm.cpu().numpy().tobytes() == means.tobytes()


# ---------------------------------------------------------------------------------------------------------------- 6. find_lines
def _search_cases(nfft, seed):
    """(spectra (S, nfft) float64, bands): every spectrum with every band"""
    rng = np.random.default_rng(seed)
    noise = rng.exponential(size=nfft)
    line = rng.exponential(size=nfft)
    line[nfft // 5 - 1:nfft // 5 + 2] *= (30.0, 200.0, 80.0)
    line[-nfft // 7] *= 150.0
    ties = rng.exponential(size=nfft)
    ties[[nfft // 8, nfft // 8 + 9, nfft - nfft // 8]] = 40.0       # equal maxima: the smallest searched bin wins
    first = rng.exponential(size=nfft)
    first[0] = 90.0                                               # its left neighbour is bin nfft - 1
    last = rng.exponential(size=nfft)
    last[nfft - 1] = 90.0                                         # its right neighbour is bin 0
    sparse = rng.exponential(size=nfft)
    sparse[rng.permutation(nfft)[:(3 * nfft) // 4]] = 0.0         # a zero median, zero neighbours
    tiny = rng.exponential(size=nfft) * 1e-300                    # subnormal neighbours of normal numbers: patterns still order
    spectra = np.stack([noise, line, ties, first, last, sparse, np.zeros(nfft), tiny])
    b = 1.0 / nfft
    bands = [(0.05, 0.3, False), (-0.3, -0.05, False), (0.0, 0.25, True), (0.1, 0.3, True), (7 * b, 7 * b, False), (-0.5, 0.5, False),
             (0.0, 0.0, False), (-b, b, False), (0.0, 9 * b, False), (0.0, 10 * b, False), (-0.5, -0.5 + 2 * b, False), (0.5 - 3 * b, 0.5, True),
             (-3 * b, 0.0, False), (0.0, 0.5, True)]
    return spectra, bands


@pytest.mark.parametrize("nfft", [64, 1024, 4096])
def test_find_lines_is_find_line_exactly(nfft):
    spectra, bands = _search_cases(nfft, seed=nfft)
    S_, B = spectra.shape[0], len(bands)
    every = np.repeat(spectra, B, axis=0)
    all_bands = bands * S_
    dev = torch.from_numpy(every).cuda()
    got = frontend.find_lines(dev, all_bands)
    rec = frontend.line_records(dev, all_bands)
    f = np.fft.fftfreq(nfft)
    counts = set()
    for i, (p, (lo, hi, two)) in enumerate(zip(every, all_bands)):
        assert got[i] == frontend.find_line(p, lo, hi, two), (nfft, i // B, i % B)
        g = np.abs(f) if two else f
        band = np.flatnonzero((g >= lo) & (g <= hi))
        k = int(band[np.argmax(p[band])])
        s = np.sort(p[band])
        r = rec[i]
        assert (int(r["bin"]), int(r["count"])) == (k, band.size) and (r["peak"], r["left"], r["right"]) == (p[k], p[(k - 1) % nfft], p[(k + 1) % nfft])
        assert (r["median_lo"], r["median_hi"]) == (s[(band.size - 1) // 2], s[band.size // 2])
        counts.add(band.size % 2)
    assert counts == {0, 1} and any(r["count"] == 1 for r in rec) and any(r["count"] == nfft for r in rec)
    assert frontend.find_lines(dev[3:4], [bands[0]])[0] == frontend.find_line(every[3], *bands[0])      # p[None], one band
    # a NaN, an infinity, a negative value: count -1 for that spectrum alone, a ValueError from find_lines; -0.0 is a zero
    bad = spectra[:5].copy()
    bad[1, nfft // 3], bad[2, 5], bad[3, nfft - 1], bad[4, 9] = np.nan, np.inf, -1e-300, -0.0
    rec = frontend.line_records(torch.from_numpy(bad).cuda(), [bands[0]] * 5)
    assert rec["count"].tolist() == [rec["count"][0], -1, -1, -1, rec["count"][0]] and rec["count"][0] > 0
    for s in (1, 2, 3):
        with pytest.raises(ValueError, match="non-finite or negative"):
            frontend.find_lines(torch.from_numpy(bad[s:s + 1]).cuda(), [bands[0]])
    assert frontend.find_lines(torch.from_numpy(bad[4:5]).cuda(), [bands[0]])[0] == frontend.find_line(bad[4], *bands[0])
    with pytest.raises(ValueError, match="spectrum 1: no bin"):
        frontend.find_lines(dev[:2], [bands[0], (0.3, 0.2, False)])
    assert frontend.find_lines(dev[:0], []) == []


# ---------------------------------------------------------------------------------------------------------------- 7. end to end
@functools.lru_cache(maxsize=None)
def _example():
    spec = importlib.util.spec_from_file_location("classify_capture", os.path.join(ROOT, "examples", "classify_capture.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    return ex


@functools.lru_cache(maxsize=None)
def _hopper():
    return _example().synthetic_hopper("ci16")                   # shared: nobody writes to it


def _same_records(batched, loop, kind):
    assert len(batched) == len(loop)
    for b, r in zip(batched, loop):
        assert list(b) == list(r)      # key for key, in the same order
        for key in r:
            if key in ("probs", "labels", "window_dbfs"):
                assert isinstance(b[key], kind) and isinstance(r[key], kind) and b[key].dtype == r[key].dtype and b[key].shape == r[key].shape, key
                assert torch.equal(b[key], r[key]) if kind is torch.Tensor else b[key].tobytes() == r[key].tobytes(), key
            else:
                assert type(b[key]) is type(r[key]) and b[key] == r[key], key


def test_detect_iq_refine_is_the_recipe_by_hand_and_batched_is_the_loop():
    """The bars are the reference's (tests/test_iq_line_spectra.py): symbol rate within 1e-3 relative, carrier within 1e-5 cycles
    per sample, the x^4 line, the plan exactly 1/4."""
    iq = _hopper()
    ex = _example()
    m = VTCNN2.synthetic("deployed3")
    dev = torch.from_numpy(iq.copy()).cuda()
    plain = m.detect_iq(dev, "ci16", dc_guard=0)
    loop = m.detect_iq(dev, "ci16", dc_guard=0, refine=True)
    assert len(plain) == len(loop) == 7
    centres = (-0.475, 0.21, 20 / 1024, -0.18, 0.475, 0.21, 0.33)      # synthetic_hopper's, in order of (first_pair, centre)
    assert all(abs(r["centre"] - c) * 1024 <= 2 for r, c in zip(loop, centres))
    for rec, before, fc in zip(loop, plain, centres):
        assert not set(FIVE) & set(before) and set(rec) - set(before) == set(FIVE)      # refine=False has none of the five keys
        assert all(rec[key] == before[key] for key in before if key not in ("shift", "interpolate", "decimate", "probs", "labels", "window_dbfs",
                                                                             "windows", "label"))
        print(f"centre {fc:+.4f}: plan {before['interpolate']}/{before['decimate']} -> {rec['interpolate']}/{rec['decimate']}, symbol rate x 32 - 1 = "
              f"{rec['symbol_rate'] * 32 - 1.0:+.2e} ({rec['symbol_line_db']:.1f} dB), carrier error {rec['centre'] + rec['carrier_offset'] - fc:+.2e} "
              f"(order {rec['carrier_order']}, {rec['carrier_line_db']:.1f} dB; centroid {rec['centre'] - fc:+.2e})")
        # by hand, with the parent's public pieces
        D0 = min(max(int(1.0 / (4.0 * rec["bandwidth"])), 1), 256)
        part = dev[2 * rec["first_pair"]:2 * rec["stop_pair"]]
        iso = frontend.ddc(part, "ci16", shift=-rec["centre"], decimate=D0, taps=frontend.plan_taps(1, D0)).reshape(-1)
        b = rec["bandwidth"] * D0
        mm = min(b / 8.0, 0.12)
        lines = []
        for order, band in ((0, (b / 2.5, min(0.45, 1.25 * b), False)), (2, (0.0, 2.0 * mm, True)), (4, (0.0, 4.0 * mm, True))):
            rows = frontend.line_spectrum(iso, "ci16", order, nfft=1024, avg=8).cpu().numpy()
            assert rows.shape[0] >= 1
            lines.append(frontend.find_line(_mean_in_row_order(rows), *band))
        (rate, rate_db), (f2, db2), (f4, db4) = lines
        assert rate_db >= 8.0 and db2 < 8.0 <= db4
        assert (rec["symbol_rate"], rec["symbol_line_db"]) == (rate / D0, rate_db)
        assert (rec["carrier_offset"], rec["carrier_order"], rec["carrier_line_db"]) == (f4 / 4 / D0, 4, db4)
        shift = -(rec["centre"] + f4 / 4 / D0)
        shift = shift - round(shift) if abs(shift) > 0.5 else shift
        L, D, _ = frontend.resample_ratio(1.0, rate / D0, 8)
        assert (rec["shift"], rec["interpolate"], rec["decimate"]) == (shift, L, D) == (shift, 1, 4)
        assert abs(rec["symbol_rate"] * 32 - 1.0) <= 1e-3 and abs(rec["centre"] + rec["carrier_offset"] - fc) <= 1e-5
        down = frontend.ddc(part, "ci16", shift=shift, decimate=D, taps=frontend.plan_taps(L, D))
        down = down[:down.shape[0] // 128 * 128]
        assert down.shape[0] >= 128
        p, l, d = m.predict_iq(down.reshape(-1), "ci16", normalize="rms", squelch_dbfs=None, return_power=True)
        assert torch.equal(rec["probs"], p) and torch.equal(rec["labels"], l) and torch.equal(rec["window_dbfs"], d)
        open_ = l[l >= 0]
        assert rec["windows"] == l.shape[0] and rec["label"] == int(torch.bincount(open_).argmax())
    # batched: the loop's records, key for key and bit for bit; a device capture and a numpy capture
    _same_records(m.detect_iq(dev, "ci16", dc_guard=0, refine=True, batched=True), loop, torch.Tensor)
    _same_records(m.detect_iq(iq, "ci16", dc_guard=0, refine=True, batched=True), m.detect_iq(iq, "ci16", dc_guard=0, refine=True), np.ndarray)
    for kw in (dict(), dict(min_line_db=99.0), dict(line_nfft=256, line_avg=2)):      # the defaults' DC guard; no line passes; other spectra
        a, z = m.detect_iq(dev, "ci16", refine=True, **kw), m.detect_iq(dev, "ci16", refine=True, batched=True, **kw)
        _same_records(z, a, torch.Tensor)
        if "min_line_db" in kw:
            base = m.detect_iq(dev, "ci16")
            assert all(r["symbol_rate"] is None and r["carrier_order"] == 0 and r["carrier_offset"] == 0.0 for r in a)
            assert [(r["shift"], r["interpolate"], r["decimate"]) for r in a] == [(r["shift"], r["interpolate"], r["decimate"]) for r in base]
    # boxes too short for one window -- and for one row of line spectra: the plan stands, the five keys say "no line"
    kw = dict(nfft=64, avg=1, min_rows=1, min_bins=1, reach_rows=0, reach_bins=0, threshold_db=8.0, refine=True)
    a, z = m.detect_iq(dev[:2 * 8192], "ci16", **kw), m.detect_iq(dev[:2 * 8192], "ci16", batched=True, **kw)
    assert len(a) >= 1 and all(r["windows"] == 0 and r["label"] == -1 and r["probs"].shape == (0, 3) for r in z)
    assert all(r["symbol_rate"] is None and r["symbol_line_db"] == float("-inf") and r["carrier_offset"] == 0.0 and r["carrier_order"] == 0
               and r["carrier_line_db"] == float("-inf") for r in z)
    _same_records(z, a, torch.Tensor)
    assert m.detect_iq(dev, "ci16", threshold_db=90.0, refine=True, batched=True) == [] == m.detect_iq(dev, "ci16", threshold_db=90.0, refine=True)
    m._release()


# ---------------------------------------------------------------------------------------------------------------- 8. the example
def test_example_refine_prints_the_same_rows_batched_and_leaves_the_plain_text_alone(capsys):
    ex = _example()
    model = VTCNN2.synthetic("deployed3")
    iq = _hopper()
    ex.detections(model, iq, "ci16")
    plain = capsys.readouterr().out
    ex.detections(model, iq, "ci16", refine=False, batched=True)
    assert capsys.readouterr().out == plain and "symbol rate" not in plain
    found = ex.detections(model, iq, "ci16", refine=True)
    loop = capsys.readouterr().out
    ex.detections(model, iq, "ci16", refine=True, batched=True)
    batched = capsys.readouterr().out
    assert batched == loop and len(loop.strip().splitlines()) == 2 + len(found)
    head, lines = loop.splitlines()[1], loop.splitlines()[2:]
    assert head.endswith(f" {'symbol rate':>12s} {'refined':>12s}") and head[:-26] == plain.splitlines()[1]
    for line, d in zip(lines, found):
        symbol = "-" if d["symbol_rate"] is None else f"{d['symbol_rate']:.6g}"
        assert line.endswith(f" {symbol:>12s} {d['centre'] + d['carrier_offset']:12.8g}")
    assert len(found) == 7 and all(" 1/4 " in line for line in lines)               # the dwells at 32 samples per symbol: 1/4 is exactly 8
    assert all(abs(d["symbol_rate"] * 32 - 1.0) <= 1e-3 for d in found)
    model._release()
