"""mdc_iq_spectrogram, mdc_iq_line_spectrum and mdc_iq_channelizer on the MI355X, held to their own rounding noise instead of the
header's worst-case bound (tests/iq_fft_f32_ref.py has the bars and their derivation, tests/test_iq_transform_noise.py the CPU
evidence that the header's bound passes coarse twiddle tables and a butterfly with its neighbour's twiddle, and that these
bars do not):

  1. sparse sweeps: a ci16 capture of 2 nfft pairs, zero except two full-range pairs d apart, hop 1 -- one call moves the first
     impulse over every position of the transform.  Every addition then has a zero operand or is the one meeting of the two
     terms; every bin of every row within sparse_bound, gamma = u (6 ceil(log2 nfft / 2) + 2), of the float64 reference.  nfft
     in {64, 128, 256, 2048, 4096} x d in {1, nfft/4 + 1, nfft/2 + 3}; one case with avg = 3; one with the staging's largest
     products;
  2. cu8 and ci8 cannot hold a zero: a full-range capture under windows that are zero except at two positions, 16 (p, q) per
     size with the seams of the first pass's butterflies and lanes, nfft 64 and 4096;
  3. line orders 0, 2 and 4 on the impulse sweep (the full-scale corner and a random pair), nfft 64, 128, 4096;
  4. dense rms: the parity tests' capture recipe, three formats, five sizes, two (hop, avg), orders 1, 0, 2, 4: per row
     row_rms(device) <= 2 x row_rms(float32 restatement of that row);
  5. channelizer, dense: outside the grey zone | |Y - floor Y| - 0.5 | <= 4 delta (delta: the restatement's largest deviation
     of the case) the output EQUALS clamp(rint(Y)); inside it is one of the two neighbours;
  6. channelizer, sparse: one or two non-zero taps on every residue, first_index 0 and 5, the same rule with the grey zone
     from sparse_bound_lsb.
Every call goes straight through the binding into a sentinel-filled output with a guard row behind it."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import iq_channelizer_ref as C                                                           # noqa: E402
import iq_fft_f32_ref as F                                                               # noqa: E402
import iq_line_ref as R                                                                  # noqa: E402
import iq_spectrum_ref as S                                                              # noqa: E402
from modulationdetectioncnn_amd import _cabi, frontend                                   # noqa: E402

SENTINEL = -7.0
CHAN_SENTINEL = -21846                                                                   # 0xAAAA
CHUNK = 512
ORDERS = [1, 0, 2, 4]


def _spectrum(iq, fmt, order, nfft, hop, avg, w, scale):
    """mdc_iq_spectrogram (order 1) or mdc_iq_line_spectrum on the flat numpy capture: the (rows, nfft) float32 numpy result
    after checking the guard row and that no sentinel is left"""
    L = _cabi.lib()
    pairs = iq.size // 2
    dev, wdev = torch.from_numpy(iq).cuda(), torch.from_numpy(w).cuda()
    rows = L.mdc_iq_spectrogram_rows(pairs, nfft, hop, avg)
    assert rows == S.rows_count(pairs, nfft, hop, avg) and rows > 0
    out = torch.full((rows + 1, nfft), SENTINEL, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    if order == 1:
        rc = L.mdc_iq_spectrogram(dev.data_ptr(), S.FMT[fmt], pairs, nfft, hop, avg, wdev.data_ptr(), scale, out.data_ptr(), rows, stream)
    else:
        rc = L.mdc_iq_line_spectrum(dev.data_ptr(), S.FMT[fmt], pairs, order, nfft, hop, avg, wdev.data_ptr(), scale, out.data_ptr(), rows,
                                    stream)
    _cabi.check(rc)
    torch.cuda.synchronize()
    assert bool((out[rows] == SENTINEL).all())
    got = out[:rows].cpu().numpy()
    assert np.all(np.isfinite(got)) and got.min() >= 0.0
    return got


def _reference(iq, fmt, order, nfft, hop, avg, w, scale, rows=None):
    if order == 1:
        return S.spectrogram(iq, fmt, nfft, hop, avg, w, scale, rows)
    return R.line_spectrum(iq, fmt, order, nfft, hop, avg, w, scale, rows)


def _sparse_score(got, iq, fmt, order, nfft, hop, avg, w, scale):
    """largest |got - P| / sparse_bound over every bin of every row, after checking that no segment stages more than two
    non-zero values and none stages none"""
    worst = 0.0
    for r0 in range(0, got.shape[0], CHUNK):
        rows = np.arange(r0, min(r0 + CHUNK, got.shape[0]))
        P, Ps, _ = _reference(iq, fmt, order, nfft, hop, avg, w, scale, rows)
        A, count = F.staged_amplitudes(iq, fmt, order, nfft, hop, avg, w, rows)
        assert 1 <= count.min() and count.max() <= 2
        worst = max(worst, float((np.abs(got[rows].astype(np.float64) - P) / F.sparse_bound(A, Ps, P, nfft, avg, scale, R.C[order])).max()))
    return worst


def _impulse_sweep(nfft, d, order=1, avg=1, pairs_at=None):
    iq = F.impulse_capture(nfft, d, seed=nfft + d, pairs_at=pairs_at)
    w = F.random_window(nfft, seed=nfft)
    scale = F.window_scale(w)
    got = _spectrum(iq, "ci16", order, nfft, 1, avg, w, scale)
    assert got.shape == ((nfft + 1) // avg, nfft)
    return _sparse_score(got, iq, "ci16", order, nfft, 1, avg, w, scale)


# ---------------------------------------------------------------------------------------------------------------- 1. sparse sweeps
@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("nfft", F.NOISE_NFFTS)
def test_impulse_sweep_within_sparse_bound(nfft, which):
    d = F.impulse_distances(nfft)[which]
    score = _impulse_sweep(nfft, d)
    print(f"nfft {nfft} d {d}: largest error / sparse_bound {score:.3f}")
    assert score <= 1.0, (nfft, d, score)


def test_impulse_sweep_with_three_segments_a_row():
    nfft = 2048
    score = _impulse_sweep(nfft, nfft // 4 + 1, avg=3)
    print(f"nfft {nfft} avg 3: largest error / sparse_bound {score:.3f}")
    assert score <= 1.0, score


def test_impulse_sweep_with_the_largest_products():
    nfft = 4096
    score = _impulse_sweep(nfft, 1, pairs_at=F.FULL_SCALE_PAIRS)
    print(f"nfft {nfft} full-scale pairs: largest error / sparse_bound {score:.3f}")
    assert score <= 1.0, score


# ---------------------------------------------------------------------------------------------------------------- 2. the window path
@pytest.mark.parametrize("nfft", [64, 4096])
@pytest.mark.parametrize("fmt", ["cu8", "ci8"])
def test_two_point_windows_within_sparse_bound(fmt, nfft):
    hop = nfft // 2
    pairs = nfft + (F.DENSE_ROWS - 1) * hop
    iq = F.dense_capture(fmt, pairs, seed=nfft)[2:2 + 2 * pairs].copy()
    worst = 0.0
    for p, q in F.sparse_windows(nfft):
        w = F.two_point_window(nfft, p, q, seed=p + q)
        scale = F.window_scale(w)
        got = _spectrum(iq, fmt, 1, nfft, hop, 1, w, scale)
        assert got.shape == (F.DENSE_ROWS, nfft)
        score = _sparse_score(got, iq, fmt, 1, nfft, hop, 1, w, scale)
        worst = max(worst, score)
        assert score <= 1.0, (fmt, nfft, p, q, score)
    print(f"{fmt} nfft {nfft}: largest error / sparse_bound {worst:.3f}")


# ---------------------------------------------------------------------------------------------------------------- 3. line orders
@pytest.mark.parametrize("nfft", [64, 128, 4096])
@pytest.mark.parametrize("order", [0, 2, 4])
def test_line_orders_within_sparse_bound(order, nfft):
    score = _impulse_sweep(nfft, nfft // 4 + 1, order=order, pairs_at=F.line_pairs(nfft))
    print(f"order {order} nfft {nfft}: largest error / sparse_bound {score:.3f}")
    assert score <= 1.0, (order, nfft, score)


# ---------------------------------------------------------------------------------------------------------------- 4. dense rms
@pytest.mark.parametrize("nfft", F.NOISE_NFFTS)
@pytest.mark.parametrize("fmt", F.FORMATS)
def test_dense_rows_are_as_quiet_as_a_float32_transform(fmt, nfft):
    """The factor 2 is over the float32 restatement of the same row, never over the kernel: two unrelated float32 algorithms
    agree within 1.5 on every one of these rows (test_iq_transform_noise.py), the kernel differs from the restatement by
    fused multiply-adds alone, and the weakest injected fault moves the statistic more than 20 times."""
    worst = 0.0
    for cfmt, n, hop, avg, pairs, seed in F.dense_cases():
        if (cfmt, n) != (fmt, nfft):
            continue
        iq = F.dense_capture(fmt, pairs, seed)[2:2 + 2 * pairs].copy()
        w = F.random_window(nfft, seed=nfft)
        scale = F.window_scale(w)
        for order in ORDERS:
            P, _, Ts = _reference(iq, fmt, order, nfft, hop, avg, w, scale)
            T = Ts.mean(axis=1)
            got = _spectrum(iq, fmt, order, nfft, hop, avg, w, scale)
            assert got.shape == P.shape == (F.DENSE_ROWS, nfft)
            ratio = F.row_rms(got, P, T) / F.row_rms(F.spectrogram_f32(iq, fmt, order, nfft, hop, avg, w, scale), P, T)
            print(f"{fmt} nfft {nfft} hop {hop} avg {avg} order {order}: row_rms device / restatement "
                  f"{ratio.min():.3f} .. {ratio.max():.3f}")
            worst = max(worst, float(ratio.max()))
            assert ratio.max() <= 2.0, (fmt, nfft, hop, avg, order, ratio)
    print(f"{fmt} nfft {nfft}: largest row_rms device / restatement {worst:.3f}")


# ---------------------------------------------------------------------------------------------------------------- 5. channelizer, dense
def _channelize(iq, fmt, first, M, D, taps, shift):
    """mdc_iq_channelizer on the flat numpy capture: the (M, n_out, 2) int16 numpy result after checking the guard row"""
    L = _cabi.lib()
    pairs, T = iq.size // 2, taps.size
    dev, hdev = torch.from_numpy(iq).cuda(), torch.from_numpy(taps).cuda()
    n_out = L.mdc_iq_channelizer_out_count(pairs, M, T, D)
    assert n_out == C.out_count(pairs, T, D) and n_out > 0
    out = torch.full((M + 1, n_out, 2), CHAN_SENTINEL, dtype=torch.int16, device="cuda")
    _cabi.check(L.mdc_iq_channelizer(dev.data_ptr(), S.FMT[fmt], pairs, first, M, D, hdev.data_ptr(), T, shift, out.data_ptr(), n_out,
                                     torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert bool((out[M] == CHAN_SENTINEL).all())
    return out[:M].cpu().numpy()


def _hold_rounding(got, Y, delta, what):
    """The rule: outside the grey zone of half-width delta the output equals clamp(rint(Y)); inside it is clamp(floor(Y)) or
    clamp(floor(Y) + 1).  Returns the grey share and the largest |got - Y| over the components the clamp does not hold."""
    assert got.shape == Y.shape + (2,)
    grey = F.grey_zone(Y, delta)
    want = C.rounded(Y)
    bad = (got != want) & ~grey
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    lo, hi = F.neighbours(Y)
    assert ((got == lo) | (got == hi))[grey].all(), what
    z = np.stack([Y.real, Y.imag], axis=2)
    free = (z > -32768.5) & (z < 32767.5)
    return float(grey.mean()), float(np.abs(got.astype(np.float64) - z)[free].max())


@functools.lru_cache(maxsize=None)
def _channel_cases():
    return list(F.channelizer_cases(frontend.design_channelizer))


@pytest.mark.parametrize("M", F.NOISE_CHANNELS)
def test_channelizer_rounds_like_the_definition_outside_the_grey_zone(M):
    greyest, furthest, clamped = 0.0, 0.0, 0
    for fmt, m, D, first, taps, shift, pairs, seed, jp in _channel_cases():
        if m != M:
            continue
        iq = F.dense_capture(fmt, pairs, seed, plant=(jp * D, taps), run=F.channelizer_run(pairs))[2:2 + 2 * pairs].copy()
        Y, _ = C.channelize(iq, fmt, first, M, D, taps, shift)
        Yh = F.channelize_f32(iq, fmt, first, M, D, taps, shift)
        delta = float(max(np.abs(Yh.real - Y.real).max(), np.abs(Yh.imag - Y.imag).max()))
        got = _channelize(iq, fmt, first, M, D, taps, shift)
        assert got.shape == (M, 37, 2)
        share, far = _hold_rounding(got, Y, 4.0 * delta, (fmt, M, D, taps.size))
        greyest, furthest = max(greyest, share), max(furthest, far)
        assert Y[0, jp].real > 32767.5 and Y[0, jp].imag < -32768.5 and tuple(got[0, jp]) == (32767, -32768)      # the clamp, both ways
        clamped += 1
    assert clamped == 12
    print(f"M {M}: largest |out - Y| outside the clamp {furthest:.4f} LSB, largest grey share {100 * greyest:.2f} %")


# ---------------------------------------------------------------------------------------------------------------- 6. channelizer, sparse
@pytest.mark.parametrize("first", [0, 5])
@pytest.mark.parametrize("M", F.SPARSE_CHANNELS)
def test_channelizer_with_one_or_two_taps(M, first):
    T, D = M + 5, 3
    pairs = T + 4 * D
    iq = F.random_capture("ci16", pairs, seed=M)
    greyest, seen = 0.0, np.zeros(M, bool)
    for t0 in range(M):
        taps, shift = F.sparse_taps(M, t0)
        vr, vi = C.branch_sums(iq, "ci16", first, M, D, taps)
        mag = np.hypot(vr.astype(np.float64), vi.astype(np.float64))
        assert ((mag != 0).sum(axis=1) <= 2).all()
        seen |= (mag != 0).any(axis=0)
        Y = F.channels_of(vr, vi, shift)
        got = _channelize(iq, "ci16", first, M, D, taps, shift)
        share, _ = _hold_rounding(got, Y, F.sparse_bound_lsb(mag.sum(axis=1), M, shift), (M, first, t0))
        greyest = max(greyest, share)
    assert seen.all()                                            # the non-zero branch sum has been every element of the transform
    print(f"M {M} first_index {first}: largest grey share {100 * greyest:.2f} %")
