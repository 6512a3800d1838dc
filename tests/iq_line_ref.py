"""float64 numpy restatement of mdc_iq_line_spectrum (include/mdc.h, "line spectrum"): the definition the tests hold the kernel
to.  Written from the header's text, not from the kernel: y in int64 integers with the magnitudes asserted, v = y w 2^-q as
float64 -- exact for orders 0, 1 and 2 (|y w| <= 2^46 < 2^53); for order 4 (|y w| <= 2^77) y w is split into a high and a low
part that are each exact, and their sum rounds once, relative error 2^-53, far below u^2 = 2^-48 -- then np.fft.fft and the
power spectrogram's bound with the header's c."""
import numpy as np

import iq_spectrum_ref as S
from iq_ddc_ref import widen

ORDERS = (0, 1, 2, 4)
Q = {0: 16, 1: 0, 2: 16, 4: 48}            # v = y w 2^-q
C = {0: 2, 1: 0, 2: 2, 4: 2}               # float32 roundings on a value before the transform (the header derives them)
Y_MAX = {0: 2 ** 31, 1: 2 ** 15, 2: 2 ** 31, 4: 2 ** 62}
U = S.U


def power_of(I, Q_, order):
    """y = (re, im) int64 arrays from the widened (I, Q) int64 arrays; every product fits: |I|, |Q| <= 2^15"""
    I, Q_ = np.asarray(I, np.int64), np.asarray(Q_, np.int64)
    assert order in ORDERS and max(np.abs(I).max(initial=0), np.abs(Q_).max(initial=0)) <= 32768
    if order == 0:
        re, im = I * I + Q_ * Q_, np.zeros_like(I)
    elif order == 1:
        re, im = I, Q_
    else:
        re, im = I * I - Q_ * Q_, 2 * I * Q_
        if order == 4:
            assert max(np.abs(re).max(initial=0), np.abs(im).max(initial=0)) <= 2 ** 31       # squares <= 2^62: inside int64
            re, im = re * re - im * im, 2 * (re * im)      # |re| <= max(a^2, b^2), |a b| <= (a^2 + b^2) / 2 <= 2^61
    assert max(np.abs(re).max(initial=0), np.abs(im).max(initial=0)) <= Y_MAX[order]
    return re, im


def _times_window(y, w, q):
    """y w 2^-q as float64; exact below 2^53, else one rounding of the sum of two exact parts"""
    if np.abs(y).max(initial=0) < 2 ** 37:
        p = y * w
        assert np.abs(p).max(initial=0) < 2 ** 53
        return p.astype(np.float64) * 2.0 ** -q
    hi, lo = y >> 32, y & 0xFFFFFFFF                        # y = hi 2^32 + lo, |hi| <= 2^30, 0 <= lo < 2^32
    return ((hi * w).astype(np.float64) * 2.0 ** 32 + (lo * w).astype(np.float64)) * 2.0 ** -q


def segment_powers(iq, fmt, order, nfft, window, scale, starts):
    """P_s[k] = scale |X_s[k]|^2 for the segments starting at the listed pairs: (len(starts), nfft) float64."""
    re, im = power_of(*widen(iq, fmt), order)
    w = np.asarray(window).astype(np.int64)
    assert w.shape == (nfft,) and np.abs(w).max(initial=0) <= 32768
    idx = np.asarray(starts, np.int64)[:, None] + np.arange(nfft, dtype=np.int64)[None, :]
    vr, vi = _times_window(re[idx], w[None, :], Q[order]), _times_window(im[idx], w[None, :], Q[order])
    assert max(np.abs(vr).max(initial=0), np.abs(vi).max(initial=0)) <= 2.0 ** 30
    X = np.fft.fft(vr + 1j * vi, axis=1)
    return float(scale) * (X.real ** 2 + X.imag ** 2)


def line_spectrum(iq, fmt, order, nfft, hop, avg, window, scale, rows=None):
    """(P, P_s, T_s) as iq_spectrum_ref.spectrogram: P[r,k] (rows, nfft), the per-segment scaled powers (rows, avg, nfft) and
    their totals over the bins (rows, avg).  rows: every row (None) or the listed row indices."""
    assert S.MIN_NFFT <= nfft <= S.MAX_NFFT and nfft & (nfft - 1) == 0 and hop >= 1 and 1 <= avg <= S.MAX_AVG
    pairs = np.asarray(iq).size // 2
    n_rows = S.rows_count(pairs, nfft, hop, avg)
    r = np.arange(n_rows, dtype=np.int64) if rows is None else np.asarray(rows, np.int64)
    assert r.size == 0 or (r.min() >= 0 and r.max() < n_rows)
    starts = ((r[:, None] * avg + np.arange(avg, dtype=np.int64)[None, :]) * hop).reshape(-1)
    Ps = segment_powers(iq, fmt, order, nfft, window, scale, starts).reshape(r.size, avg, nfft)
    return Ps.mean(axis=1), Ps, Ps.sum(axis=2)


def bound(P, Ps, Ts, nfft, avg, order):
    """The power spectrogram's bound with eps = u (8 (log2 nfft + 1) + c): c = 2 for orders 0, 2 and 4 -- the exact integer y
    rounds once when it becomes a float32 (|y| is not below 2^24), w 2^-q is exact, their product rounds once more; by Parseval
    a relative perturbation c u of every v moves every bin by at most c u sqrt(T_s / scale) -- and c = 0 for order 1."""
    eps = U * (8.0 * (np.log2(nfft) + 1.0) + C[order])
    T = Ts[:, :, None]
    return (2.0 * eps * np.sqrt(Ps * T) + eps * eps * T).mean(axis=1) + (avg + 4) * U * P


def line_psd(iq, fmt, order, nfft, avg, window, scale):
    """What frontend's estimators look at: the hop = nfft / 2 line spectrum, rows of `avg` segments, all rows averaged: (nfft,)
    float64, or None when the capture is too short for one row"""
    pairs = np.asarray(iq).size // 2
    segs = S.rows_count(pairs, nfft, nfft // 2, avg) * avg
    if segs == 0:
        return None
    acc = np.zeros(nfft)
    for s0 in range(0, segs, 256):
        starts = np.arange(s0, min(segs, s0 + 256), dtype=np.int64) * (nfft // 2)
        acc += segment_powers(iq, fmt, order, nfft, window, scale, starts).sum(axis=0)
    return acc / segs
