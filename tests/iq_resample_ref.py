"""numpy int64 restatement of mdc_iq_resample (include/mdc.h, "rational resampler"): the definition the tests hold the kernel
to, bit for bit.  Written from the header's text, not from the kernel: the mixed samples of iq_ddc_ref.mix are zero-stuffed
LITERALLY (v_{nL} = m_n, zeros between, none after the last sample) and filtered by iq_ddc_ref.fir_decimate, the header's
sum_k h_k v_{jD+k} with its rounding and clamp.  No polyphase branch is ever formed here, except to check the precondition."""
import numpy as np

import iq_ddc_ref as D

FMT, DTYPE, SAMPLE_MIN, SAMPLE_MAX = D.FMT, D.DTYPE, D.SAMPLE_MIN, D.SAMPLE_MAX
MAX_INTERPOLATE, MAX_DECIMATE, MAX_TAPS, MAX_BRANCH_ABS_SUM = 32, 256, 1024, 65535


def out_count(pairs, ntaps, interpolate, decimate):
    if pairs < 1:
        return 0
    lv = (pairs - 1) * interpolate + 1
    return (lv - ntaps) // decimate + 1 if lv >= ntaps else 0


def branch_abs_sums(taps, interpolate):
    """sum_i |h_{r + iL}| for r = 0 .. L-1 (0 for a branch without taps)"""
    h = np.abs(np.asarray(taps).astype(np.int64))
    return [int(h[r::interpolate].sum()) for r in range(interpolate)]


def check_taps(taps, interpolate):
    h = np.asarray(taps)
    assert h.dtype.kind == "i" and h.ndim == 1 and 1 <= h.size <= MAX_TAPS
    h = h.astype(np.int64)
    assert h.min() >= -32768 and h.max() <= 32767
    sums = branch_abs_sums(h, interpolate)
    assert max(sums) <= MAX_BRANCH_ABS_SUM, sums
    return h


def stuff(m, interpolate):
    """v of length (P - 1) L + 1 with v[nL] = m[n]; an empty capture stays empty"""
    if m.size == 0:
        return m
    v = np.zeros((m.size - 1) * interpolate + 1, np.int64)
    v[::interpolate] = m
    return v


def resample(iq, fmt, phase0, step, interpolate, decimate, taps, n0=0, outputs=None):
    """The whole chain: (n_out, 2) int16 (or one row per listed output index).  n0: the index of the capture's first pair in the
    oscillator's count."""
    L, Dm = int(interpolate), int(decimate)
    assert 1 <= L <= MAX_INTERPOLATE and 1 <= Dm <= MAX_DECIMATE
    h = check_taps(taps, L)
    m_re, m_im = D.mix(iq, fmt, phase0, step, n0)
    v_re, v_im = stuff(m_re, L), stuff(m_im, L)
    assert D.out_count(v_re.size, h.size, Dm) == out_count(m_re.size, h.size, L, Dm)
    return np.stack([D.fir_decimate(v_re, h, Dm, outputs), D.fir_decimate(v_im, h, Dm, outputs)], axis=1).astype(np.int16)


def resample_sparse(iq, fmt, phase0, step, interpolate, decimate, taps, outputs):
    """resample for a few listed outputs of a LARGE capture: output j reads v_{jD} .. v_{jD+T-1}; only the input pairs that
    stretch of v holds are mixed, and the stretch is stuffed as literally as the whole would be."""
    L, Dm = int(interpolate), int(decimate)
    h = check_taps(taps, L)
    a = np.asarray(iq).reshape(-1, 2)
    T = h.size
    n_out = out_count(a.shape[0], T, L, Dm)
    rows = np.empty((len(outputs), 2), np.int16)
    for row, j in enumerate(outputs):
        assert 0 <= j < n_out
        lo = j * Dm                                          # the stretch of v: lo .. lo + T - 1
        first, last = -(-lo // L), (lo + T - 1) // L         # the input pairs n with lo <= nL <= lo + T - 1
        acc = np.zeros(2, np.int64)
        if last >= first:
            m_re, m_im = D.mix(a[first: last + 1].reshape(-1), fmt, phase0, step, n0=first)
            v = np.zeros((2, T), np.int64)
            at = np.arange(first, last + 1) * L - lo
            v[0, at], v[1, at] = m_re, m_im
            acc = (v * h[None, :]).sum(axis=1)
        assert np.abs(acc).max() + 8192 < 2 ** 31
        rows[row] = np.clip((acc + 8192) >> 14, -32768, 32767)
    return rows
