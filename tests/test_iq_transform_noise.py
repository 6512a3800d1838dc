"""How much of a wrong transform the header's worst-case bound lets through, and the two tighter bars that catch it -- all on the
CPU, from tests/iq_fft_f32_ref.py (float32 numpy restatements of the kernels' transform) against the float64 references.
tests/test_iq_transform_noise_gpu.py holds the kernels to the same bars; this file is what those bars rest on:

  1. both float32 algorithms stay inside the header's bounds (iq_spectrum_ref.bound, iq_line_ref.bound,
     iq_channelizer_ref.bound) on the GPU tests' capture recipe at the smallest and the largest size;
  2. their row_rms agree within a factor 1.5 on every row of every dense case of the GPU file, their largest channelizer
     deviations within a factor 2: the measurement the GPU file's margins (2 and 4) rest on;
  3. the gap, shown: each injected fault passes the header's bound in a named case of the existing GPU grid, scores > 1 under
     sparse_bound on the impulse sweep and moves row_rms by more than the GPU file's factor 2;
  4. the sparse fixtures are what the derivation assumes (<= 2 non-zero staged values, every position and every twiddle entry
     of every pass visited) and the clean restatement stays below half the bound;
  5. the channelizer's grey zone holds <= 5 % of the outputs of every case, and outside it the restatement rounds to the
     definition's integer everywhere.
Run with -s for the tables; DESIGN.md 5.17-5.19 quote them."""
import functools

import numpy as np
import pytest

import iq_channelizer_ref as C
import iq_fft_f32_ref as F
import iq_line_ref as L
import iq_spectrum_ref as S
from modulationdetectioncnn_amd import frontend

ORDERS = [1, 0, 2, 4]
CHUNK = 512


def _reference(iq, fmt, order, nfft, hop, avg, w, scale, rows=None):
    if order == 1:
        return S.spectrogram(iq, fmt, nfft, hop, avg, w, scale, rows)
    return L.line_spectrum(iq, fmt, order, nfft, hop, avg, w, scale, rows)


def _header_bound(P, Ps, Ts, nfft, avg, order):
    return S.bound(P, Ps, Ts, nfft, avg) if order == 1 else L.bound(P, Ps, Ts, nfft, avg, order)


@functools.lru_cache(maxsize=None)
def _dense(fmt, nfft, hop, avg, pairs, seed, order):
    """one dense case: the capture, the window, the float64 reference and both float32 restatements"""
    iq = F.dense_capture(fmt, pairs, seed)[2:2 + 2 * pairs]
    w = F.random_window(nfft, seed=nfft)
    scale = F.window_scale(w)
    P, Ps, Ts = _reference(iq, fmt, order, nfft, hop, avg, w, scale)
    assert P.shape == (F.DENSE_ROWS, nfft)
    a = F.spectrogram_f32(iq, fmt, order, nfft, hop, avg, w, scale)
    b = F.spectrogram_f32(iq, fmt, order, nfft, hop, avg, w, scale, fft=F.fft_radix2)
    return iq, w, scale, P, Ps, Ts, a, b


@functools.lru_cache(maxsize=None)
def _channel_cases():
    return list(F.channelizer_cases(frontend.design_channelizer))


@functools.lru_cache(maxsize=None)
def _channel(i):
    fmt, M, D, first, taps, shift, pairs, seed, jp = _channel_cases()[i]
    iq = F.dense_capture(fmt, pairs, seed, plant=(jp * D, taps), run=F.channelizer_run(pairs))[2:2 + 2 * pairs]
    Y, Sj = C.channelize(iq, fmt, first, M, D, taps, shift)
    assert Y.shape == (M, 37)
    a = F.channelize_f32(iq, fmt, first, M, D, taps, shift)
    b = F.channelize_f32(iq, fmt, first, M, D, taps, shift, fft=F.fft_radix2)
    return Y, Sj, a, b


def _deviation(Yh, Y):
    """largest |Y^ - Y| over the components, in output LSB"""
    return float(max(np.abs(Yh.real - Y.real).max(), np.abs(Yh.imag - Y.imag).max()))


# ---------------------------------------------------------------------------------------------------------------- 1. inside the header
def test_restatements_stay_inside_the_headers_bounds():
    worst = 0.0
    for fmt, nfft, hop, avg, pairs, seed in F.dense_cases():
        if nfft not in (F.NOISE_NFFTS[0], F.NOISE_NFFTS[-1]):
            continue
        for order in ORDERS:
            _, _, _, P, Ps, Ts, a, b = _dense(fmt, nfft, hop, avg, pairs, seed, order)
            bound = _header_bound(P, Ps, Ts, nfft, avg, order)
            for got in (a, b):
                ratio = float((np.abs(got - P) / bound).max())
                worst = max(worst, ratio)
                assert ratio <= 1.0, (fmt, nfft, hop, avg, order, ratio)
    print(f"spectra: largest restatement error / header bound {worst:.4f}")
    worst = 0.0
    for i, (fmt, M, D, first, taps, shift, pairs, seed, jp) in enumerate(_channel_cases()):
        if M not in (F.NOISE_CHANNELS[0], F.NOISE_CHANNELS[-1]):
            continue
        Y, Sj, a, b = _channel(i)
        re, im = C.clamped(Y)
        for Yh in (a, b):
            out = C.rounded(Yh).astype(np.float64)
            err = np.maximum(np.abs(out[:, :, 0] - re), np.abs(out[:, :, 1] - im))
            ratio = float((err / C.bound(Sj, M)[None, :]).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (fmt, M, D, ratio)
    print(f"channelizer: largest restatement error / header bound {worst:.4f}")


# ---------------------------------------------------------------------------------------------------------------- 2. two algorithms
def test_the_two_float32_algorithms_agree():
    """What the GPU file's factor 2 (rms) and 4 (grey zone) rest on: two unrelated float32 algorithms differ by less than 1.5 in
    row_rms on every row, and by less than 2 in a channelizer case's largest deviation."""
    worst, per_size = 1.0, {}
    for fmt, nfft, hop, avg, pairs, seed in F.dense_cases():
        for order in ORDERS:
            _, _, _, P, Ps, Ts, a, b = _dense(fmt, nfft, hop, avg, pairs, seed, order)
            T = Ts.mean(axis=1)
            ra, rb = F.row_rms(a, P, T), F.row_rms(b, P, T)
            assert ra.min() > 0 and rb.min() > 0
            ratio = float(np.maximum(ra / rb, rb / ra).max())
            worst = max(worst, ratio)
            lo, hi = per_size.get(nfft, (np.inf, 0.0))
            per_size[nfft] = (min(lo, ra.min() / F.U), max(hi, ra.max() / F.U))
            assert ratio <= 1.5, (fmt, nfft, hop, avg, order, ratio)
    for nfft, (lo, hi) in per_size.items():
        print(f"nfft {nfft}: row_rms of the radix-4 restatement {lo:.4f} .. {hi:.4f} u")
    print(f"row_rms, radix-4 Stockham against recursive radix-2: largest ratio {worst:.3f}")
    worst, inside = 1.0, 1.0
    for i, case in enumerate(_channel_cases()):
        Y, _, a, b = _channel(i)
        da, db = _deviation(a, Y), _deviation(b, Y)
        ratio = max(da / db, db / da)
        worst = max(worst, ratio)
        assert ratio <= 2.0, (case[:4], da, db)
        # the case's maximum sits in the planted, clamping column, where the branch sums' conversion to float32 -- common to
        # both -- is most of it; the outputs the clamp does not hold tell the transforms apart
        free = (np.abs(Y.real) < 32768) & (np.abs(Y.imag) < 32768)
        fa, fb = _deviation(a[free], Y[free]), _deviation(b[free], Y[free])
        inside = max(inside, fa / fb, fb / fa)
        assert max(fa / fb, fb / fa) <= 2.0, (case[:4], fa, fb)
    print(f"channelizer, largest |Y^ - Y| of a case, one algorithm against the other: largest ratio {worst:.3f} "
          f"(over the outputs inside the int16 range alone: {inside:.3f})")


# ---------------------------------------------------------------------------------------------------------------- 3. the gap
def _sweep(nfft, d, order=1, avg=1, fault=F.NO_FAULT, pairs_at=None, met=None, stop_above=None):
    """the impulse sweep in float32 against the float64 reference: largest |P^ - P| / sparse_bound over all rows (or, with
    stop_above, over the chunks of rows up to the first that exceeds it) and the largest count of non-zero staged values in a
    segment.  met: a list that receives fft_stockham4's record of the twiddle entries met, united over the rows."""
    iq = F.impulse_capture(nfft, d, seed=nfft + d, pairs_at=pairs_at)
    w = F.random_window(nfft, seed=nfft)
    scale = F.window_scale(w)
    n_rows = S.rows_count(2 * nfft, nfft, 1, avg)
    worst, most, hits = 0.0, 0, [] if met is not None else None
    for r0 in range(0, n_rows, CHUNK):
        rows = np.arange(r0, min(r0 + CHUNK, n_rows))
        P, Ps, _ = _reference(iq, "ci16", order, nfft, 1, avg, w, scale, rows)
        A, count = F.staged_amplitudes(iq, "ci16", order, nfft, 1, avg, w, rows)
        most = max(most, int(count.max()))
        assert count.min() >= 1
        chunk_met = [] if met is not None else None
        got = F.spectrogram_f32(iq, "ci16", order, nfft, 1, avg, w, scale, rows, fault=fault, met=chunk_met)
        if met is not None:
            hits = chunk_met if not hits else [h | c for h, c in zip(hits, chunk_met)]
        worst = max(worst, float((np.abs(got - P) / F.sparse_bound(A, Ps, P, nfft, avg, scale, L.C[order])).max()))
        if stop_above is not None and worst > stop_above:
            break
    if met is not None:
        met.extend(hits)
    return worst, most


@functools.lru_cache(maxsize=None)
def _clean_sweep(nfft, d):
    """(score, most, met) of the clean restatement on the (nfft, d) sweep: shared by the fault table and the fixture test"""
    met = []
    score, most = _sweep(nfft, d, met=met)
    return score, most, met


def _grid_case(nfft, fmt="ci16"):
    """a named case of tests/test_iq_spectrogram_gpu.py's parity grid: (hop, avg) = (nfft/2, 3), 5 rows, its random window"""
    hop, avg = nfft // 2, 3
    pairs = nfft + (5 * avg - 1) * hop
    iq = F.dense_capture(fmt, pairs, seed=nfft + hop + pairs)[2:2 + 2 * pairs]
    w = np.random.default_rng(nfft).integers(0, 32768, size=nfft).astype(np.int16)
    return iq, fmt, nfft, hop, avg, w, F.window_scale(w)


@pytest.mark.parametrize("nfft", [2048, 4096])
def test_faults_pass_the_header_and_fail_the_new_bars(nfft):
    """Every fault of iq_fft_f32_ref.faults is caught by the sparse sweep (score > 1) and by the rms rule (> 2 x the clean
    restatement on some row); the gap is those of them that the header's bound lets through in the existing grid's ci16,
    (nfft/2, 3) case -- both coarse tables, and at 4096 the neighbour's twiddle in the first pass (2 pi / 4096 of phase)."""
    iq, fmt, _, hop, avg, w, scale = _grid_case(nfft)
    P, Ps, Ts = S.spectrogram(iq, fmt, nfft, hop, avg, w, scale)
    bound = S.bound(P, Ps, Ts, nfft, avg)
    header = lambda f: float((np.abs(F.spectrogram_f32(iq, fmt, 1, nfft, hop, avg, w, scale, fault=f) - P) / bound).max())
    dfmt, dn, dhop, davg, dpairs, dseed = next(c for c in F.dense_cases() if c[0] == "ci16" and c[1] == nfft and c[3] == 1)
    diq, dw, dscale, dP, _, dTs, clean, _ = _dense(dfmt, dn, dhop, davg, dpairs, dseed, 1)
    rms_clean = F.row_rms(clean, dP, dTs.mean(axis=1))
    d = nfft // 4 + 1
    print(f"\nnfft {nfft}: fault | error / header bound (ci16, hop nfft/2, avg 3) | error / sparse_bound (d = {d}) | row_rms / clean")
    print(f"  none | {header(F.NO_FAULT):.4f} | {_clean_sweep(nfft, d)[0]:.3f} | 1")
    weakest_sparse, weakest_rms, shown = np.inf, np.inf, 0
    for fault in F.faults(nfft):
        h = header(fault)
        shown += h <= 1.0
        full = fault.twiddle_bits is not None          # a coarse table is wrong in every row; one butterfly only in a few
        sparse, _ = _sweep(nfft, d, fault=fault, stop_above=None if full else 1.0)
        got = F.spectrogram_f32(diq, dfmt, 1, dn, dhop, davg, dw, dscale, fault=fault)
        rms = float((F.row_rms(got, dP, dTs.mean(axis=1)) / rms_clean).max())
        note, least = "" if h <= 1.0 else " (caught: not part of the gap)", "" if full else ">= "
        print(f"  {fault.name} | {h:.3f}{note} | {least}{sparse:.3g} | {rms:.3g}")
        assert sparse > 1.0, (nfft, fault, sparse)
        assert rms > 2.0, (nfft, fault, rms)
        if h <= 1.0:
            weakest_sparse, weakest_rms = min(weakest_sparse, sparse), min(weakest_rms, rms)
    assert shown >= (3 if nfft == 4096 else 2), shown      # both coarse tables; at 4096 the first pass's neighbour as well
    print(f"  weakest detection: {weakest_sparse:.3g} x sparse_bound, {weakest_rms:.3g} x the clean row_rms (the bar is 2)")


@pytest.mark.parametrize("nfft", [64, 128, 256])
def test_coarse_tables_pass_the_header_at_small_sizes_too(nfft):
    """16- and 18-bit twiddles pass the header's bound at every size; the small sizes' sweeps catch them as well."""
    iq, fmt, _, hop, avg, w, scale = _grid_case(nfft)
    P, Ps, Ts = S.spectrogram(iq, fmt, nfft, hop, avg, w, scale)
    for fault in F.faults(nfft)[:2]:
        h = float((np.abs(F.spectrogram_f32(iq, fmt, 1, nfft, hop, avg, w, scale, fault=fault) - P) / S.bound(P, Ps, Ts, nfft, avg)).max())
        sparse = min(_sweep(nfft, d, fault=fault)[0] for d in F.impulse_distances(nfft))
        print(f"nfft {nfft} {fault.name}: error / header bound {h:.3f}, error / sparse_bound (smallest over d) {sparse:.3f}")
        assert h <= 1.0 and sparse > 1.0, (nfft, fault, h, sparse)


# ---------------------------------------------------------------------------------------------------------------- 4. the fixtures
@pytest.mark.parametrize("nfft", F.NOISE_NFFTS)
def test_impulse_sweep_is_what_the_derivation_assumes(nfft):
    worst = 0.0
    for d in F.impulse_distances(nfft):
        score, most, met = _clean_sweep(nfft, d)
        assert most <= 2
        # row r has the first impulse at nfft - 1 - r: rows 0 .. nfft - 1 are every position once (the capture has 2 nfft pairs,
        # hop 1: nfft + 1 rows)
        assert S.rows_count(2 * nfft, nfft, 1, 1) == nfft + 1
        assert len(met) == F.twiddled_passes(nfft)
        for p, hit in enumerate(met):                  # every entry the pass reads (the multiples of its stride), in all three tables
            assert np.array_equal(hit, np.broadcast_to(F.pass_entries(nfft, p), hit.shape)), (nfft, d, p, int(hit.sum()))
        assert score < 0.5, (nfft, d, score)
        worst = max(worst, score)
    print(f"nfft {nfft}: clean restatement / sparse_bound {worst:.3f}")
    if nfft == 2048:                                   # the GPU file's case with three segments a row
        score, most = _sweep(nfft, nfft // 4 + 1, avg=3)
        assert most <= 2 and score < 0.5, score
        print(f"nfft {nfft}, avg 3: {score:.3f}")
    if nfft == 4096:                                   # and its case with the staging's largest products
        score, most = _sweep(nfft, 1, pairs_at=F.FULL_SCALE_PAIRS)
        assert most <= 2 and score < 0.5, score
        print(f"nfft {nfft}, full-scale pairs: {score:.3f}")


@pytest.mark.parametrize("nfft", [64, 128, 4096])
@pytest.mark.parametrize("order", [0, 2, 4])
def test_line_orders_on_the_impulse_sweep(order, nfft):
    """a zero pair stages to zero at every order, order 0 stages a real value, and the full-scale pair reaches order 4's 64-bit
    range; the staging's two roundings enter sparse_bound as iq_line_ref.C"""
    d = nfft // 4 + 1
    iq = F.impulse_capture(nfft, d, pairs_at=F.line_pairs(nfft))
    I, Q = F.widen(iq, "ci16")
    vr, vi = F.stage(I, Q, np.full(I.size, 32767), order)
    assert int(((vr != 0) | (vi != 0)).sum()) == 2 and (order != 0 or not vi.any())
    if order == 4:
        yr, yi = L.power_of(I, Q, 4)
        assert max(np.abs(yr).max(), np.abs(yi).max()) == 2 ** 62
    score, most = _sweep(nfft, d, order=order, pairs_at=F.line_pairs(nfft))
    assert most <= 2 and score < 0.5, (order, nfft, score)
    print(f"order {order} nfft {nfft}: clean restatement / sparse_bound {score:.3f}")


@pytest.mark.parametrize("nfft", [64, 4096])
@pytest.mark.parametrize("fmt", ["cu8", "ci8"])
def test_two_point_windows_are_sparse(fmt, nfft):
    """cu8 and ci8 cannot hold a zero: the window does.  Full-range capture, 16 windows that are zero except at (p, q)."""
    hop = nfft // 2
    pairs = nfft + (F.DENSE_ROWS - 1) * hop
    iq = F.dense_capture(fmt, pairs, seed=nfft)[2:2 + 2 * pairs]
    worst = 0.0
    for p, q in F.sparse_windows(nfft):
        w = F.two_point_window(nfft, p, q, seed=p + q)
        scale = F.window_scale(w)
        P, Ps, _ = S.spectrogram(iq, fmt, nfft, hop, 1, w, scale)
        A, count = F.staged_amplitudes(iq, fmt, 1, nfft, hop, 1, w)
        assert count.max() <= 2 and count.min() >= 1                         # cu8 widens to odd multiples of 128: never zero
        got = F.spectrogram_f32(iq, fmt, 1, nfft, hop, 1, w, scale)
        worst = max(worst, float((np.abs(got - P) / F.sparse_bound(A, Ps, P, nfft, 1, scale)).max()))
    assert worst < 0.5, (fmt, nfft, worst)
    print(f"{fmt} nfft {nfft}: clean restatement / sparse_bound {worst:.3f}")


@pytest.mark.parametrize("M", F.SPARSE_CHANNELS)
def test_sparse_taps_are_sparse(M):
    """one or two non-zero taps give one or two non-zero branch sums per column, on every residue over the sweep, and the clean
    restatement stays below half of sparse_bound_lsb"""
    worst, seen = 0.0, np.zeros(M, bool)
    T, D = M + 5, 3
    pairs = T + 4 * D
    iq = F.random_capture("ci16", pairs, seed=M)
    for first in (0, 5):
        sums, shifts = [], set()
        for t0 in range(M):
            taps, shift = F.sparse_taps(M, t0)
            vr, vi = C.branch_sums(iq, "ci16", first, M, D, taps)
            assert ((np.hypot(vr.astype(np.float64), vi.astype(np.float64)) != 0).sum(axis=1) <= 2).all()
            sums.append((vr, vi))
            shifts.add(shift)
        vr, vi = np.concatenate([v[0] for v in sums]), np.concatenate([v[1] for v in sums])      # every tap set's columns in one transform
        (shift,) = shifts
        mag = np.hypot(vr.astype(np.float64), vi.astype(np.float64))
        seen |= (mag != 0).any(axis=0)
        Y, Yh = F.channels_of(vr, vi, shift), F.channels_f32_of(vr, vi, shift)
        bound = F.sparse_bound_lsb(mag.sum(axis=1), M, shift)[None, :]
        assert bound.min() > 0
        worst = max(worst, float((np.maximum(np.abs(Yh.real - Y.real), np.abs(Yh.imag - Y.imag)) / bound).max()))
    assert seen.all() and worst < 0.5, (M, worst)
    print(f"M {M}: clean restatement / sparse_bound_lsb {worst:.3f}")


# ---------------------------------------------------------------------------------------------------------------- 5. the grey zone
def test_channelizer_grey_zone_is_thin_and_the_rest_is_exact():
    """Per dense case: delta = the restatement's largest |Y^ - Y|; the zone | |Y - floor Y| - 0.5 | <= 4 delta holds <= 5 % of
    the outputs, and outside it the restatement rounds to the definition's integer without exception."""
    most, widest = 0.0, 0.0
    for i, case in enumerate(_channel_cases()):
        Y, _, a, _ = _channel(i)
        delta = _deviation(a, Y)
        grey = F.grey_zone(Y, 4.0 * delta)
        share = float(grey.mean())
        most, widest = max(most, share), max(widest, delta)
        assert share <= 0.05, (case[:4], case[5], share, delta)
        assert np.array_equal(C.rounded(a)[~grey], C.rounded(Y)[~grey]), case[:4]
        lo, hi = F.neighbours(Y)
        out = C.rounded(a)
        assert ((out == lo) | (out == hi))[grey].all(), case[:4]
    print(f"channelizer: largest delta {widest:.5f} LSB, largest grey share {100 * most:.2f} %")
