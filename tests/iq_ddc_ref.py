"""numpy int64 restatement of mdc_iq_ddc (include/mdc.h, "digital down-converter"): the definition the tests hold the kernel
to, bit for bit.  Written from the header's text, not from the kernel; every intermediate is an int64 array, and the ranges the
32-bit device arithmetic relies on are asserted on every call."""
import numpy as np

CU8, CI8, CI16 = 0, 1, 2
FMT = {"cu8": CU8, "ci8": CI8, "ci16": CI16}
DTYPE = {"cu8": np.uint8, "ci8": np.int8, "ci16": np.dtype("<i2")}
SAMPLE_MIN = {"cu8": 0, "ci8": -128, "ci16": -32768}
SAMPLE_MAX = {"cu8": 255, "ci8": 127, "ci16": 32767}
NCO_ENTRIES = 4096
MAX_DECIMATE, MAX_TAPS, MAX_TAPS_ABS_SUM = 256, 1024, 65535


def nco_table():
    """(4096, 2) int16: c_k = rint(32767 cos(2 pi k / 4096)), s_k = rint(32767 sin(2 pi k / 4096))."""
    a = 2.0 * np.pi * np.arange(NCO_ENTRIES, dtype=np.float64) / NCO_ENTRIES
    t = np.stack([np.rint(32767.0 * np.cos(a)), np.rint(32767.0 * np.sin(a))], axis=1)
    assert np.abs(t).max() <= 32767
    return t.astype(np.int16)


_TABLE = nco_table().astype(np.int64)


def out_count(pairs, ntaps, decimate):
    return (pairs - ntaps) // decimate + 1 if pairs >= ntaps else 0


def widen(iq, fmt):
    """flat interleaved samples of the format's dtype -> (I, Q) int64 at 16-bit full scale"""
    a = np.asarray(iq)
    assert a.dtype == np.dtype(DTYPE[fmt]), (a.dtype, fmt)
    s = a.astype(np.int64).reshape(-1, 2)
    if fmt == "cu8":
        s = (2 * s - 255) * 128
    elif fmt == "ci8":
        s = s * 256
    assert np.abs(s).max(initial=0) <= 32768
    return s[:, 0], s[:, 1]


def phases(n0, count, phase0, step):
    """phi_n = (phase0 + n step) mod 2^32 for n = n0 .. n0 + count - 1, in Python-width integers reduced before numpy sees them"""
    n = np.arange(n0, n0 + count, dtype=np.uint64)
    return (np.uint64(phase0 % (1 << 32)) + (n % np.uint64(1 << 32)) * np.uint64(step % (1 << 32))) % np.uint64(1 << 32)


def mix(iq, fmt, phase0, step, n0=0):
    """m = x e^{+j phi} / 2 as (m_re, m_im) int64, |m| <= 32767; n0: the index of the first pair (phi counts from it)"""
    I, Q = widen(iq, fmt)
    k = (phases(n0, I.size, phase0, step) >> np.uint64(20)).astype(np.int64)
    c, s = _TABLE[k, 0], _TABLE[k, 1]
    pre_re, pre_im = I * c - Q * s + 32768, I * s + Q * c + 32768
    assert max(np.abs(pre_re).max(initial=0), np.abs(pre_im).max(initial=0)) < 2 ** 31
    m_re, m_im = pre_re >> 16, pre_im >> 16            # arithmetic shifts (numpy's >> on int64 floors)
    assert max(np.abs(m_re).max(initial=0), np.abs(m_im).max(initial=0)) <= 32767
    return m_re, m_im


def check_taps(taps):
    h = np.asarray(taps)
    assert h.dtype.kind == "i" and h.ndim == 1 and 1 <= h.size <= MAX_TAPS
    h = h.astype(np.int64)
    assert h.min() >= -32768 and h.max() <= 32767
    assert int(np.abs(h).sum()) <= MAX_TAPS_ABS_SUM, int(np.abs(h).sum())
    return h


def fir_decimate(m, h, decimate, outputs=None):
    """acc_j = sum_k h_k m_{jD+k} for every j (or the listed ones), then clamp((acc + 8192) >> 14) -> int64"""
    T, D = h.size, int(decimate)
    n_out = out_count(m.size, T, D)
    j = np.arange(n_out, dtype=np.int64) if outputs is None else np.asarray(outputs, np.int64)
    assert j.size == 0 or (j.min() >= 0 and j.max() < n_out)
    acc = np.zeros(j.size, np.int64)
    if j.size * T <= 1 << 22:
        acc = (m[j[:, None] * D + np.arange(T)[None, :]] * h[None, :]).sum(axis=1) if j.size else acc
    else:                        # tap by tap: no (outputs x taps) matrix
        for k in range(T):
            acc += h[k] * m[j * D + k]
    assert np.abs(acc).max(initial=0) + 8192 < 2 ** 31
    return np.clip((acc + 8192) >> 14, -32768, 32767)


def ddc(iq, fmt, phase0, step, decimate, taps, n0=0, outputs=None):
    """The whole chain: (n_out, 2) int16 (or one row per listed output index).  1 <= D <= 256, 1 <= T <= 1024."""
    assert 1 <= int(decimate) <= MAX_DECIMATE
    h = check_taps(taps)
    m_re, m_im = mix(iq, fmt, phase0, step, n0)
    return np.stack([fir_decimate(m_re, h, decimate, outputs), fir_decimate(m_im, h, decimate, outputs)], axis=1).astype(np.int16)


def ddc_sparse(iq, fmt, phase0, step, decimate, taps, outputs):
    """ddc for a few listed outputs of a LARGE capture: only the input pairs those outputs read are mixed."""
    h = check_taps(taps)
    a = np.asarray(iq).reshape(-1, 2)
    D, T = int(decimate), h.size
    rows = np.empty((len(outputs), 2), np.int16)
    for r, j in enumerate(outputs):
        seg = a[j * D: j * D + T].reshape(-1)
        m_re, m_im = mix(seg, fmt, phase0, step, n0=j * D)
        acc = np.array([(h * m_re).sum(), (h * m_im).sum()], np.int64)
        assert np.abs(acc).max() + 8192 < 2 ** 31
        rows[r] = np.clip((acc + 8192) >> 14, -32768, 32767)
    return rows
