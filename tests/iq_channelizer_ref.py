"""float64 numpy restatement of mdc_iq_channelizer (include/mdc.h, "channelizer"): the definition the tests hold the kernel to.
Written from the header's text, not from the kernel: the branch sums as exact int64 integers (asserted below 2^31), np.fft.fft
over the residues, Y left unrounded in output LSB (already times 2^-(15+s)), and per column S_j = sqrt(sum_k |Y_j[k]|^2) in the
same unit -- what the header's error bound is stated in."""
import numpy as np

from iq_ddc_ref import DTYPE, FMT, SAMPLE_MAX, SAMPLE_MIN, widen      # noqa: F401  (the widening is mdc_iq_ddc's, word for word)

MIN_CHANNELS, MAX_CHANNELS, MAX_TAPS_PER_CHANNEL, MAX_SHIFT, MAX_BRANCH_ABS_SUM = 8, 1024, 16, 15, 65535
U = 2.0 ** -24


def out_count(pairs, ntaps, decimate):
    return (pairs - ntaps) // decimate + 1 if pairs >= ntaps else 0


def check_taps(taps, channels):
    h = np.asarray(taps)
    assert h.dtype.kind == "i" and h.ndim == 1 and 1 <= h.size <= MAX_TAPS_PER_CHANNEL * channels
    h = h.astype(np.int64)
    assert h.min() >= -32768 and h.max() <= 32767
    for r in range(min(channels, h.size)):
        assert int(np.abs(h[r::channels]).sum()) <= MAX_BRANCH_ABS_SUM, (r, int(np.abs(h[r::channels]).sum()))
    return h


def branch_sums(iq, fmt, first_index, channels, decimate, taps, columns=None):
    """v_j[r] as (re, im) int64 arrays of shape (columns, M), for every output column (None) or the listed ones"""
    M, D = int(channels), int(decimate)
    assert MIN_CHANNELS <= M <= MAX_CHANNELS and M & (M - 1) == 0 and 1 <= D <= M and first_index >= 0
    h = check_taps(taps, M)
    T = h.size
    I, Q = widen(iq, fmt)
    n_out = out_count(I.size, T, D)
    j = np.arange(n_out, dtype=np.int64) if columns is None else np.asarray(columns, np.int64)
    assert j.size == 0 or (j.min() >= 0 and j.max() < n_out)
    vr, vi = np.zeros((j.size, M), np.int64), np.zeros((j.size, M), np.int64)
    rows = np.arange(j.size)[:, None]
    for t0 in range(0, T, M):                                 # M consecutive taps meet M different residues: a plain indexed += is exact
        t = np.arange(t0, min(t0 + M, T), dtype=np.int64)[None, :]
        n = j[:, None] * D + t
        r = (int(first_index) + n) % M
        vr[rows, r] += h[t] * I[n]
        vi[rows, r] += h[t] * Q[n]
    assert max(np.abs(vr).max(initial=0), np.abs(vi).max(initial=0)) < 2 ** 31
    return vr, vi


def channelize(iq, fmt, first_index, channels, decimate, taps, tap_shift, columns=None):
    """(Y, S): Y (M, columns) complex128, UNROUNDED, in output LSB (the transform times 2^-(15+s)), channel-major like out_dev;
    S (columns,) float64 = sqrt(sum_k |Y_j[k]|^2)."""
    assert 0 <= int(tap_shift) <= MAX_SHIFT
    vr, vi = branch_sums(iq, fmt, first_index, channels, decimate, taps, columns)
    Y = np.fft.fft(vr.astype(np.float64) + 1j * vi.astype(np.float64), axis=1) * 2.0 ** -(15 + int(tap_shift))
    return Y.T.copy(), np.sqrt((Y.real ** 2 + Y.imag ** 2).sum(axis=1))


def clamped(Y):
    """clamp(Y) component-wise to the int16 range, unrounded: (re, im) float64"""
    return np.clip(Y.real, -32768.0, 32767.0), np.clip(Y.imag, -32768.0, 32767.0)


def rounded(Y):
    """the definition's output: clamp(rint(Y)) as (M, columns, 2) int16"""
    re, im = clamped(np.rint(Y.real) + 1j * np.rint(Y.imag))
    return np.stack([re, im], axis=2).astype(np.int16)


def bound(S, channels):
    """The largest |out - clamp(Y)| the header allows per column: 0.5 (the final rounding) + eps S_j, u = 2^-24,
    eps = 8u (log2 M + 1) -- the spectrogram's bound in amplitude form (clamping never increases a difference)."""
    return 0.5 + 8.0 * U * (np.log2(channels) + 1.0) * S
