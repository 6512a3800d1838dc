"""float32 numpy restatements of what the three transform kernels compute -- mdc_iq_spectrogram, mdc_iq_line_spectrum and
mdc_iq_channelizer -- and the bars tests/test_iq_transform_noise*.py hold the kernels to.  Where tests/iq_spectrum_ref.py,
iq_line_ref.py and iq_channelizer_ref.py are the float64 DEFINITION and the header's worst-case bound, this file is the
kernels' own rounding noise: the same operation count in the same number format, every operation rounded on its own (numpy
never fuses a multiply into an add), real and imaginary parts kept as separate float32 arrays.

  fft_stockham4   the passes as the head of csrc/iq_fft.h describes them: Stockham autosort, decimation in
                  frequency, radix 4, a last radix-2 pass for an odd log2 n, the three tables w^j, w^2j, w^3j read from the first
                  quadrant of the 4096-point circle as tools/gen_fft_twiddles.py rounds it.  n = 8 .. 4096.
  fft_radix2      an unrelated algorithm in the same format: plain recursive radix 2, decimation in time.
  Fault           the ways a transform can be subtly wrong that the tests inject into fft_stockham4.
  stage           the staging of mdc_iq_spectrogram (order 1) and of line orders 0, 2 and 4 with their two roundings.
  spectrogram_f32 staging, transform, |X|^2, the sum over `avg` segments in order, the gain: one row as the kernel forms it.
  channelize_f32  the transform of iq_channelizer_ref.branch_sums times 2^-(15+s), unrounded, in output LSB.
  sparse_bound    the derived bar for segments with at most two non-zero staged values.
  row_rms         the statistic of the dense comparison.
  the fixtures    the captures, windows and case lists the CPU and the GPU file share, so that "every case the GPU file uses"
                  is one list."""
import dataclasses

import numpy as np

import iq_channelizer_ref as C
import iq_line_ref as L
import iq_spectrum_ref as S
from iq_ddc_ref import widen

U = 2.0 ** -24
F32 = np.float32
CIRCLE, QUADRANT = 4096, 1024


# ------------------------------------------------------------------------------------------------------------ twiddles
def quadrant_table():
    """(1024, 2) float32: cos, sin of 2 pi j / 4096 rounded from float64 -- tools/gen_fft_twiddles.py's formula"""
    a = 2.0 * np.pi * np.arange(QUADRANT, dtype=np.float64) / CIRCLE
    return np.stack([np.cos(a), np.sin(a)], axis=1).astype(F32)


def circle_twiddle(J, bits=None):
    """e^{-2 pi i J / 4096} for 0 <= J < 3072 as (re, im) float32 arrays, from the first quadrant by swaps and sign changes;
    bits: the table's entries rounded to that many mantissa bits first (a fault)"""
    t = quadrant_table()
    if bits is not None:
        t = round_to_bits(t, bits)
    J = np.asarray(J)
    assert J.min(initial=0) >= 0 and J.max(initial=0) < 3 * QUADRANT
    j, quadrant = J & (QUADRANT - 1), J >> 10
    c, s = t[j, 0], t[j, 1]
    re = np.where(quadrant == 0, c, np.where(quadrant == 1, -s, -c))
    im = np.where(quadrant == 0, -s, np.where(quadrant == 1, -c, s))
    return re.astype(F32), im.astype(F32)


def round_to_bits(x, bits):
    """float32 values rounded to nearest with `bits` significant bits (24 changes nothing): relative error <= 2^-bits"""
    m, e = np.frexp(np.asarray(x, np.float64))
    return np.ldexp(np.rint(np.ldexp(m, bits)), e - bits).astype(F32)


def passes(n):
    """passes of the radix-4 transform with a last radix-2 pass for an odd log2: ceil(log2 n / 2)"""
    log2n = int(n).bit_length() - 1
    assert 1 << log2n == n and 8 <= n <= CIRCLE
    return (log2n + 1) // 2


# ------------------------------------------------------------------------------------------------------------ faults
@dataclasses.dataclass(frozen=True)
class Fault:
    """What is wrong with the transform.  twiddle_bits: the quadrant table keeps that many mantissa bits.  neighbour = (pass, t):
    butterfly t of that twiddled pass takes the three twiddles of the next butterfly that has other ones (index j + stride;
    j - stride at the table's end): its phases are off by 2 pi stride k / n."""
    name: str = "none"
    twiddle_bits: int = None
    neighbour: tuple = None


NO_FAULT = Fault()


def twiddled_passes(n):
    """radix-4 passes that multiply by twiddles (the last radix-4 pass of an even log2 and the radix-2 pass do not)"""
    log2n = int(n).bit_length() - 1
    return log2n // 2 if log2n & 1 else log2n // 2 - 1


def pass_entries(n, p):
    """(n/4,) bool: the entries j of the tables w^j, w^2j, w^3j that twiddled pass p reads -- the multiples of its stride 4^p"""
    return np.arange(n // 4) % (1 << (2 * p)) == 0


def faults(n):
    """every fault the tests inject at size n: the two coarse tables and the neighbour's twiddle once per twiddled pass"""
    out = [Fault("twiddles to 16 bits", twiddle_bits=16), Fault("twiddles to 18 bits", twiddle_bits=18)]
    for p in range(twiddled_passes(n)):
        out.append(Fault(f"neighbour's twiddle, pass {p}", neighbour=(p, (n // 4) // 3)))
    return out


# ------------------------------------------------------------------------------------------------------------ the transforms
def _cmul(ar, ai, wr, wi):
    return ar * wr - ai * wi, ar * wi + ai * wr            # four products, two sums, each rounded to float32


def fft_stockham4(vr, vi, fault=NO_FAULT, met=None):
    """The kernels' transform of (segments, n) float32 arrays (re, im): (Xr, Xi) float32 in natural order.
    met: a list that receives, per twiddled pass, a (3, n/4) bool array -- which entry of w^j, w^2j, w^3j met a non-zero
    operand in some segment."""
    xr, xi = np.array(vr, F32), np.array(vi, F32)
    assert xr.ndim == 2 and xr.shape == xi.shape
    n = xr.shape[1]
    log2n = n.bit_length() - 1
    assert 1 << log2n == n and 8 <= n <= CIRCLE
    NB, odd = n // 4, bool(log2n & 1)
    t = np.arange(NB)
    tw = [circle_twiddle(k * t * (CIRCLE // n), fault.twiddle_bits) for k in (1, 2, 3)]
    for p in range(twiddled_passes(n)):
        s = 1 << (2 * p)
        ar, ai, br, bi = xr[:, :NB], xi[:, :NB], xr[:, NB:2 * NB], xi[:, NB:2 * NB]
        cr, ci, dr, di = xr[:, 2 * NB:3 * NB], xi[:, 2 * NB:3 * NB], xr[:, 3 * NB:], xi[:, 3 * NB:]
        apcr, apci, amcr, amci = ar + cr, ai + ci, ar - cr, ai - ci
        bpdr, bpdi = br + dr, bi + di
        jr, ji = -(bi - di), br - dr                                         # i (b - d)
        j = t & ~(s - 1)
        if fault.neighbour is not None and fault.neighbour[0] == p:
            j = j.copy()
            bt = fault.neighbour[1]
            j[bt] = j[bt] + s if j[bt] + s < NB else j[bt] - s
        pre = [(amcr - jr, amci - ji), (apcr - bpdr, apci - bpdi), (amcr + jr, amci + ji)]
        if met is not None:
            hit = np.zeros((3, NB), bool)
            for k in range(3):
                np.logical_or.at(hit[k], j, ((pre[k][0] != 0) | (pre[k][1] != 0)).any(axis=0))
            met.append(hit)
        y = [(apcr + bpdr, apci + bpdi)] + [_cmul(pre[k][0], pre[k][1], tw[k][0][j], tw[k][1][j]) for k in range(3)]
        q = t & (s - 1)
        base = q + 4 * (t - q)
        nr, ni = np.empty_like(xr), np.empty_like(xi)
        for k in range(4):
            nr[:, base + k * s], ni[:, base + k * s] = y[k]
        xr, xi = nr, ni
    if not odd:                                                              # the last radix-4 pass: bins t + k n/4
        ar, ai, br, bi = xr[:, :NB], xi[:, :NB], xr[:, NB:2 * NB], xi[:, NB:2 * NB]
        cr, ci, dr, di = xr[:, 2 * NB:3 * NB], xi[:, 2 * NB:3 * NB], xr[:, 3 * NB:], xi[:, 3 * NB:]
        apcr, apci, amcr, amci = ar + cr, ai + ci, ar - cr, ai - ci
        bpdr, bpdi = br + dr, bi + di
        jr, ji = -(bi - di), br - dr
        return (np.concatenate([apcr + bpdr, amcr - jr, apcr - bpdr, amcr + jr], axis=1),
                np.concatenate([apci + bpdi, amci - ji, apci - bpdi, amci + ji], axis=1))
    h = n // 2                                                               # the last radix-2 pass: bins t and t + n/2
    return (np.concatenate([xr[:, :h] + xr[:, h:], xr[:, :h] - xr[:, h:]], axis=1),
            np.concatenate([xi[:, :h] + xi[:, h:], xi[:, :h] - xi[:, h:]], axis=1))


def fft_radix2(vr, vi):
    """A structurally different float32 transform: recursive radix 2, decimation in time, X[k] = E[k] + w_n^k O[k], its
    twiddles e^{-2 pi i k / n} rounded from float64 per level."""
    xr, xi = np.asarray(vr, F32), np.asarray(vi, F32)
    n = xr.shape[1]
    if n == 1:
        return xr.copy(), xi.copy()
    er, ei = fft_radix2(xr[:, 0::2], xi[:, 0::2])
    orr, oi = fft_radix2(xr[:, 1::2], xi[:, 1::2])
    a = -2.0 * np.pi * np.arange(n // 2, dtype=np.float64) / n
    tr, ti = _cmul(orr, oi, np.cos(a).astype(F32), np.sin(a).astype(F32))
    return np.concatenate([er + tr, er - tr], axis=1), np.concatenate([ei + ti, ei - ti], axis=1)


def power(xr, xi):
    """|X|^2 as the kernel's norm2: two squares and their sum, float32"""
    return xr * xr + xi * xi


# ------------------------------------------------------------------------------------------------------------ staging
def stage(I, Q, w, order):
    """The staged values of include/mdc.h ("power spectrogram", "line spectrum") in float32, (re, im): order 1 converts the
    exact integer product (one rounding); orders 0, 2 and 4 convert the exact integer y (the first rounding) and multiply by
    w 2^-q, itself exact (the second).  I, Q: widened int64 arrays; w: the window's values, broadcast against them."""
    I, Q, w = np.asarray(I, np.int64), np.asarray(Q, np.int64), np.asarray(w, np.int64)
    if order == 1:
        return (I * w).astype(F32), (Q * w).astype(F32)
    yr, yi = L.power_of(I, Q, order)
    f = w.astype(F32) * F32(2.0 ** -L.Q[order])
    return yr.astype(F32) * f, yi.astype(F32) * f


def staged_exact(I, Q, w, order):
    """the same values without rounding, float64 (re, im): what sparse_bound's amplitudes are taken from"""
    I, Q, w = np.asarray(I, np.int64), np.asarray(Q, np.int64), np.asarray(w, np.int64)
    yr, yi = L.power_of(I, Q, order)
    return L._times_window(yr, w, L.Q[order]), L._times_window(yi, w, L.Q[order])


def _starts(pairs, nfft, hop, avg, rows):
    n_rows = S.rows_count(pairs, nfft, hop, avg)
    r = np.arange(n_rows, dtype=np.int64) if rows is None else np.asarray(rows, np.int64)
    return r, ((r[:, None] * avg + np.arange(avg, dtype=np.int64)[None, :]) * hop).reshape(-1)


def spectrogram_f32(iq, fmt, order, nfft, hop, avg, window, scale, rows=None, fft=fft_stockham4, **kw):
    """One call of mdc_iq_spectrogram (order 1) or mdc_iq_line_spectrum in float32: (rows, nfft) float32.  Staging, transform,
    |X|^2, the segments of a row summed in order from 0, times gain = float32(scale / avg)."""
    I, Q = widen(iq, fmt)
    r, starts = _starts(I.size, nfft, hop, avg, rows)
    idx = starts[:, None] + np.arange(nfft, dtype=np.int64)[None, :]
    vr, vi = stage(I[idx], Q[idx], np.asarray(window)[None, :], order)
    p = power(*fft(vr, vi, **kw)).reshape(r.size, avg, nfft)
    acc = np.zeros((r.size, nfft), F32)
    for s in range(avg):
        acc = acc + p[:, s]
    return acc * F32(float(scale) / avg)


def staged_amplitudes(iq, fmt, order, nfft, hop, avg, window, rows=None):
    """(A, count): per segment the sum of |v| over the staged values, exact, (rows, avg) float64 -- sparse_bound's amplitude --
    and how many staged values of the segment are non-zero, (rows, avg)"""
    I, Q = widen(iq, fmt)
    r, starts = _starts(I.size, nfft, hop, avg, rows)
    idx = starts[:, None] + np.arange(nfft, dtype=np.int64)[None, :]
    vr, vi = staged_exact(I[idx], Q[idx], np.asarray(window)[None, :], order)
    mag = np.hypot(vr, vi)
    return mag.sum(axis=1).reshape(r.size, avg), (mag != 0).sum(axis=1).reshape(r.size, avg)


def channelize_f32(iq, fmt, first_index, channels, decimate, taps, tap_shift, columns=None, fft=fft_stockham4, **kw):
    """mdc_iq_channelizer before its final rounding: the exact branch sums converted to float32, transformed, times 2^-(15+s)
    (exact): (M, columns) complex128 holding float32 values, in output LSB, channel-major like iq_channelizer_ref.channelize"""
    return channels_f32_of(*C.branch_sums(iq, fmt, first_index, channels, decimate, taps, columns), tap_shift, fft=fft, **kw)


def channels_f32_of(vr, vi, tap_shift, fft=fft_stockham4, **kw):
    """channelize_f32 from branch sums already at hand, (columns, M) int64 each"""
    xr, xi = fft(vr.astype(F32), vi.astype(F32), **kw)
    f = F32(2.0 ** -(15 + int(tap_shift)))
    return ((xr * f).astype(np.float64) + 1j * (xi * f).astype(np.float64)).T.copy()


def channels_of(vr, vi, tap_shift):
    """iq_channelizer_ref.channelize's Y from branch sums already at hand (the sparse sweeps compute them once per tap set):
    float64 np.fft.fft over the residues times 2^-(15+s), (M, columns) complex128"""
    return (np.fft.fft(vr.astype(np.float64) + 1j * vi.astype(np.float64), axis=1) * 2.0 ** -(15 + int(tap_shift))).T.copy()


# ------------------------------------------------------------------------------------------------------------ the bars
def gamma(n, c=0):
    """u (6 ceil(log2 n / 2) + 2 + c): see sparse_bound"""
    return U * (6 * passes(n) + 2 + c)


def sparse_bound(A, Ps, P, n, avg, scale, c=0):
    """The largest |P^ - P| of a float32 transform on segments with AT MOST TWO non-zero staged values a and b, per row and bin.
    A: |a| + |b| per segment, (rows, avg), in staged units; Ps: the exact scaled powers per segment, (rows, avg, n); P their
    mean, (rows, n); c: float32 roundings on a value before the transform beyond the first (iq_line_ref.C: 2 for orders 0, 2, 4).

    Derivation (u = 2^-24, the unit roundoff; every quantity complex, errors relative to |a| and |b|).  A decimation-in-
    frequency pass splits the transform into independent sub-transforms, and a lone non-zero input of a butterfly leaves it
    as that input times 1, -1, i or -i (the other operand of every addition in it is zero: exact) times a twiddle.  So until
    the two terms meet, each travels alone:
      * one complex product per pass that has twiddles (all but the last): a float32 complex product has relative error
        <= sqrt(5) u, and the twiddle itself, two components each rounded once from float64, <= sqrt(2) u: 3.65 u per pass;
      * the two terms sit in the same butterfly in exactly one pass (their positions agree modulo the sub-transform's quarter
        from that pass on, at the latest in the last one); there each output is one addition of two non-zero values, relative
        error u of a sum no larger than |a| + |b|.  Afterwards the sum travels as one term.  Charging an addition in EVERY
        pass, 4.65 u per pass, is already more than happens;
      * before the transform the integer's conversion to float32, u (plus c u for the line orders' two staging roundings, which
        iq_line_ref.bound counts as 2 on top of it); after it the squares and their sum, <= 1.5 u of the power, and the product
        with gain, 0.5 u more: together u in amplitude.
    With p = ceil(log2 n / 2) passes: |X^ - X| <= u (4.65 p + 2 + c) (|a| + |b|) to first order; gamma = u (6 p + 2 + c) leaves
    1.35 u per pass for the second-order terms and for a compiler's fused multiply-adds, which round once where this model
    rounds twice and can only do better.  gamma depends on n through p alone.  In power:
        |P^_s - P_s| <= 2 gamma A sqrt(scale P_s) + scale gamma^2 A^2,
    the mean over the row's segments, and (avg - 1) u P for the avg - 1 additions of the row's sum."""
    g = gamma(n, c)
    A = np.asarray(A, np.float64)[:, :, None]
    return (2.0 * g * A * np.sqrt(float(scale) * Ps) + float(scale) * (g * A) ** 2).mean(axis=1) + (avg - 1) * U * P


def sparse_bound_lsb(A, M, tap_shift):
    """the channelizer's form: |Y^ - Y| <= gamma(M) A 2^-(15+s) per component, in output LSB; A = |v1| + |v2| per column, the
    branch sums' magnitudes.  (gamma's allowance for the squares covers the scaling, which is exact.)"""
    return gamma(M) * np.asarray(A, np.float64) * 2.0 ** -(15 + int(tap_shift))


def row_rms(P_hat, P, T):
    """rms over the bins of (P^ - P) / (2 sqrt(P T)), per row: (rows,) float64.  P^ = |X + e|^2 gives P^ - P = 2 Re(conj(X) e)
    + |e|^2, so the quotient is the error's component along X in units of sqrt(T), the scale a float32 transform's error
    really has on dense input.  T: the row's total power (rows,) -- for avg > 1 the mean of its segments' totals.  Bins with
    P == 0 are left out."""
    P_hat, P = np.asarray(P_hat, np.float64), np.asarray(P, np.float64)
    T = np.asarray(T, np.float64).reshape(-1, 1)
    ok = P > 0
    q = np.where(ok, (P_hat - P) / (2.0 * np.sqrt(np.where(ok, P, 1.0) * T)), 0.0)
    return np.sqrt((q * q).sum(axis=1) / ok.sum(axis=1))


def grey_zone(Y, delta):
    """(M, columns, 2) bool: components of the unrounded Y (output LSB) whose fraction lies within `delta` of a half -- where a
    float32 transform may legitimately round to the other neighbour.  delta: a scalar or one value per column."""
    z = np.stack([Y.real, Y.imag], axis=2)
    d = np.broadcast_to(np.asarray(delta, np.float64), (Y.shape[1],)) if np.ndim(delta) else float(delta)
    d = d[None, :, None] if np.ndim(d) else d
    return np.abs(np.abs(z - np.floor(z)) - 0.5) <= d


def neighbours(Y):
    """the two integers an output in the grey zone may be: clamp(floor(Y)), clamp(floor(Y) + 1), each (M, columns, 2) int16"""
    z = np.floor(np.stack([Y.real, Y.imag], axis=2))
    return np.clip(z, -32768, 32767).astype(np.int16), np.clip(z + 1, -32768, 32767).astype(np.int16)


# ------------------------------------------------------------------------------------------------------------ shared fixtures
FORMATS = ["cu8", "ci8", "ci16"]
NOISE_NFFTS = [64, 128, 256, 2048, 4096]      # 16 busy lanes / even log2; the same, odd; one butterfly per thread; the largest
#                                               odd log2; two butterflies per thread
NOISE_CHANNELS = [8, 16, 64, 128, 1024]       # the smallest; 64 transforms side by side; even; odd log2 with the two-butterfly
#                                               radix-2 pass; the largest
SPARSE_CHANNELS = [8, 16, 128, 1024]
DENSE_ROWS = 5


def dense_capture(fmt, pairs, seed, plant=None, run=300):
    """The capture recipe of tests/test_iq_spectrogram_gpu.py and test_iq_channelizer_gpu.py: one pair of padding + `pairs`
    pairs + one pair of padding.  Uniform over the whole range; from the middle on two off-bin tones, 0.6 and 0.006 of full
    scale; runs of `run` = 300 pairs of all minimum, all maximum and alternating minimum / maximum pairs at pairs 0, 700, 1500 and
    200 before the end.  plant = (at, taps): from pair `at` on I is the maximum where the tap is >= 0 and the minimum where it is
    negative, Q the opposite (the channelizer's clamping column)."""
    lo, hi, dt = S.SAMPLE_MIN[fmt], S.SAMPLE_MAX[fmt], S.DTYPE[fmt]
    rng = np.random.default_rng(seed)
    buf = rng.integers(lo, hi + 1, size=2 * (pairs + 2)).astype(dt)
    body = buf[2:2 + 2 * pairs]
    half = pairs // 2
    n = np.arange(half, pairs)
    z = 0.6 * np.exp(2j * np.pi * (0.1234567 * n + 0.3)) + 0.006 * np.exp(-2j * np.pi * (0.3141593 * n + 0.1))
    mid, amp = (lo + hi) / 2.0, (hi - lo) / 2.0
    body[2 * half:] = np.clip(np.rint(np.stack([z.real, z.imag], axis=1) * amp + mid), lo, hi).astype(dt).reshape(-1)
    alt = np.empty(4 * ((run + 1) // 2), dt)
    alt[0::4], alt[1::4], alt[2::4], alt[3::4] = lo, lo, hi, hi
    for at, level in ((0, np.full(2 * run, lo, dt)), (700, np.full(2 * run, hi, dt)), (1500, alt[:2 * run]),
                      (max(0, pairs - 200), np.full(2 * run, lo, dt))):
        seg = body[2 * at: 2 * at + 2 * run]
        seg[:] = level[:seg.size]
    if plant is not None:
        at, taps = plant
        if at + taps.size <= pairs:
            seg = body[2 * at: 2 * (at + taps.size)]
            seg[0::2] = np.where(taps >= 0, hi, lo)
            seg[1::2] = np.where(taps >= 0, lo, hi)
    return buf


def random_window(nfft, seed):
    """asymmetric, no zero entry: a reversed or shifted index shows, and no staged value vanishes by the window's doing"""
    return np.random.default_rng(seed).integers(1, 32768, size=nfft).astype(np.int16)


def window_scale(w):
    """frontend.window_scale's formula: a full-scale tone on a bin reads 1.0"""
    return 1.0 / (32768.0 * float(np.asarray(w, np.int64).sum())) ** 2


def dense_cases():
    """(fmt, nfft, hop, avg, pairs, seed) of the dense rms comparison: 5 rows each"""
    for fmt in FORMATS:
        for nfft in NOISE_NFFTS:
            for hop, avg in ((nfft // 2, 1), (nfft + 3, 2)):
                pairs = nfft + (DENSE_ROWS * avg - 1) * hop
                yield fmt, nfft, hop, avg, pairs, nfft + hop + pairs


def impulse_capture(nfft, d, seed=None, pairs_at=None):
    """flat ci16 capture of 2 nfft pairs, all zero except two pairs at nfft - 1 and nfft - 1 + d: full-range random ones, or
    the listed two.  With hop 1 row r sees them at positions nfft - 1 - r and nfft - 1 - r + d."""
    iq = np.zeros(4 * nfft, np.dtype("<i2"))
    if pairs_at is None:
        rng = np.random.default_rng(seed)
        pairs_at = rng.integers(-32768, 32768, size=(2, 2))
        pairs_at[pairs_at == 0] = 1
    for at, (i, q) in zip((nfft - 1, nfft - 1 + d), pairs_at):
        iq[2 * at], iq[2 * at + 1] = i, q
    return iq


def impulse_distances(nfft):
    return [1, nfft // 4 + 1, nfft // 2 + 3]


FULL_SCALE_PAIRS = ((-32768, -32768), (32767, -32768))      # the staging's largest products


def line_pairs(nfft):
    """the line orders' two impulses: the full-scale corner (order 2 reaches 2^31, order 4's 64-bit squares 2^62) and a
    full-range random pair"""
    i, q = (int(v) for v in np.random.default_rng(nfft).integers(-32768, 32768, size=2))
    return ((-32768, -32768), (i or 1, q or 1))


def random_capture(fmt, pairs, seed):
    """flat, uniform over the format's whole range, nothing planted"""
    return np.random.default_rng(seed).integers(S.SAMPLE_MIN[fmt], S.SAMPLE_MAX[fmt] + 1, size=2 * pairs).astype(S.DTYPE[fmt])


def sparse_windows(nfft):
    """16 (p, q): the window's only two non-zero positions.  The first four are the seams between the four elements of a
    first-pass butterfly and between lanes; the rest random."""
    fixed = [(0, nfft - 1), (0, 1), (nfft // 4 - 1, nfft // 4), (nfft // 2, nfft // 2 + 1)]
    rng = np.random.default_rng(nfft)
    while len(fixed) < 16:
        p, q = sorted(int(v) for v in rng.integers(0, nfft, size=2))
        if p != q and (p, q) not in fixed:
            fixed.append((p, q))
    return fixed


def two_point_window(nfft, p, q, seed):
    w = np.zeros(nfft, np.int16)
    w[[p, q]] = np.random.default_rng(seed).integers(8192, 32768, size=2)
    return w


def random_taps(M, T, seed):
    """test_iq_channelizer_gpu.py's: asymmetric int16 taps scaled so that the largest residue's sum |h| is just inside 65535"""
    h = np.random.default_rng(seed).integers(-32768, 32768, size=T).astype(np.float64)
    worst = max(np.abs(h[r::M]).sum() for r in range(min(M, T)))
    q = np.trunc(h * min(1.0, 65535.0 / worst)).astype(np.int16)
    C.check_taps(q, M)
    return q


def channelizer_run(pairs):
    """The dense channelizer cases' constant runs: 300 pairs as in the parity test, but never more than a sixteenth of the
    capture.  The parity test's small captures lie mostly inside such runs (M = 8, D = 3: 18 of 37 columns see one constant
    input); their outputs repeat a handful of values up to the rotation, and whichever of those lies near a half counts many
    times over -- 11 % of the outputs in a grey zone whose width predicts 2.4 %.  That says nothing about the transform."""
    return min(300, pairs // 16)


def channelizer_cases(design_channelizer):
    """(fmt, M, D, first, taps, shift, pairs, seed, planted column) of the dense channelizer comparison: n_out = 37; the capture
    is dense_capture(fmt, pairs, seed, plant=(20 D, taps), run=channelizer_run(pairs)).  The ragged random taps take
    tap_shift = log2 M, one more than the parity test gives them: the planted column then reaches twice the clamp instead of
    four times, and float32's spacing at the case's largest |Y| -- which is what delta measures -- leaves the grey zone under
    its 5 %.
    design_channelizer: frontend's (this file imports numpy only)."""
    for M in NOISE_CHANNELS:
        h, shift = design_channelizer(M)
        for taps, s in ((h, shift), (random_taps(M, 3 * M + 5, seed=M), int(np.log2(M)))):
            for fmt in FORMATS:
                for D in (M, 3):
                    first, pairs = 5, taps.size + 36 * D
                    yield fmt, M, D, first, taps, s, pairs, M + D + pairs + first, 20


def sparse_taps(M, t0):
    """(taps, shift): T = M + 5 taps, zero except at t0 (every t0 < M: every residue, every lane and element of the quad
    loads) and, for an odd t0, at a second one M/4 + 1 further (another residue: two non-zero branch sums)."""
    T = M + 5
    rng = np.random.default_rng(1000 * M + t0)
    h = np.zeros(T, np.int16)
    h[t0] = rng.choice([-1, 1]) * rng.integers(16384, 32768)
    if t0 & 1:
        h[(t0 + M // 4 + 1) % T] = rng.choice([-1, 1]) * rng.integers(16384, 32768)
    return h, 2
