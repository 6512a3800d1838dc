"""numpy int64 restatement of mdc_iq_balance_stats, the host design and mdc_iq_balance (include/mdc.h, "I/Q balance"): the
definition the tests hold the kernels and frontend.design_balance / image_rejection_db to.  Written from the header's text,
not from the kernels; every intermediate is an int64 array or a Python integer, and the ranges the device arithmetic relies on
are asserted on every call.  The widening is iq_ddc_ref's."""
import math

import numpy as np

from iq_ddc_ref import DTYPE, FMT, SAMPLE_MAX, SAMPLE_MIN, widen      # noqa: F401

MIN_BLOCK, MAX_BLOCK = 64, 1 << 20
ONE = 16384                                   # Q14
MAX_DC, MAX_ROW = 32768, 32767
IDENTITY = (0, 0, ONE, 0, 0, ONE)
SWAP = (0, 0, 0, ONE, ONE, 0)
CONJUGATE = (0, 0, ONE, 0, 0, -ONE)


def blocks(pairs, B):
    assert pairs >= 0 and MIN_BLOCK <= B <= MAX_BLOCK
    return -(-pairs // B)


def stats(iq, fmt, B):
    """(nblocks, 5) int64: sum x, sum y, sum x^2, sum y^2, sum x y over the widened pairs [b B, min((b + 1) B, pairs))"""
    x, y = widen(iq, fmt)
    nb = blocks(x.size, B)
    out = np.zeros((nb, 5), np.int64)
    if nb == 0:
        return out
    starts = np.arange(nb, dtype=np.int64) * B
    for k, v in enumerate((x, y, x * x, y * y, x * y)):
        assert np.abs(v).max() <= 2 ** 30
        out[:, k] = np.add.reduceat(v, starts)      # |sum| <= 2^20 * 2^30: exact in int64
    return out


def totals(sums, pairs):
    """(n, Sx, Sy, Sxx, Syy, Sxy) in Python integers from block rows or one summed row"""
    rows = np.asarray(sums).reshape(-1, 5)
    return (int(pairs),) + tuple(sum(int(v) for v in rows[:, k]) for k in range(5))


def central(sums, pairs):
    n, Sx, Sy, Sxx, Syy, Sxy = totals(sums, pairs)
    return n * Sxx - Sx * Sx, n * Syy - Sy * Sy, n * Sxy - Sx * Sy


def image_rejection_db(sums, pairs):
    cxx, cyy, cxy = central(sums, pairs)
    if cxx + cyy <= 0:
        return math.inf
    rho = math.hypot(cxx - cyy, 2 * cxy) / (cxx + cyy)
    if rho == 0.0:
        return math.inf
    rho = min(rho, 1.0)
    r = (1.0 - math.sqrt(1.0 - rho * rho)) / rho
    return -20.0 * math.log10(r if r > 0.0 else rho / 2.0)


def design(sums, pairs):
    """(dc_i, dc_q, m00, m01, m10, m11, scale): dc round half up; M = sqrt(tr C / 2) C^(-1/2) by eigendecomposition, Q14; scale
    is what M was multiplied by to bring both rows' absolute sums to <= 32767 (1.0: nothing)"""
    n, Sx, Sy, _, _, _ = totals(sums, pairs)
    if n == 0:
        return IDENTITY + (1.0,)
    dc = ((2 * Sx + n) // (2 * n), (2 * Sy + n) // (2 * n))
    assert max(abs(dc[0]), abs(dc[1])) <= MAX_DC
    cxx, cyy, cxy = central(sums, pairs)
    if cxx <= 0 or cyy <= 0 or cxx * cyy - cxy * cxy <= 0:
        return dc + IDENTITY[2:] + (1.0,)
    n2 = float(n) ** 2
    C = np.array([[cxx / n2, cxy / n2], [cxy / n2, cyy / n2]], np.float64)
    w, V = np.linalg.eigh(C)
    M = math.sqrt(np.trace(C) / 2.0) * (V @ np.diag(w ** -0.5) @ V.T)
    scale = 1.0
    while True:
        m = np.rint(ONE * scale * M).astype(np.int64)
        worst = int(np.abs(m).sum(axis=1).max())
        if worst <= MAX_ROW:
            return dc + (int(m[0, 0]), int(m[0, 1]), int(m[1, 0]), int(m[1, 1]), scale)
        scale *= (MAX_ROW - 0.5) / worst


def check_coeffs(c):
    dc_i, dc_q, m00, m01, m10, m11 = (int(v) for v in tuple(c)[:6])
    assert abs(dc_i) <= MAX_DC and abs(dc_q) <= MAX_DC
    assert abs(m00) + abs(m01) <= MAX_ROW and abs(m10) + abs(m11) <= MAX_ROW
    return dc_i, dc_q, m00, m01, m10, m11


def correct(iq, fmt, coeffs):
    """(pairs, 2) int16: clamp((m a + m' b + 8192) >> 14) per rail, a = x - dc_i, b = y - dc_q"""
    dc_i, dc_q, m00, m01, m10, m11 = check_coeffs(coeffs)
    x, y = widen(iq, fmt)
    a, b = x - dc_i, y - dc_q
    assert max(np.abs(a).max(initial=0), np.abs(b).max(initial=0)) <= 65536
    pre_i, pre_q = m00 * a + m01 * b + 8192, m10 * a + m11 * b + 8192
    assert max(np.abs(pre_i).max(initial=0), np.abs(pre_q).max(initial=0)) < 2 ** 31
    return np.stack([np.clip(pre_i >> 14, -32768, 32767), np.clip(pre_q >> 14, -32768, 32767)], axis=1).astype(np.int16)


def closed_form_irr_db(gain_db, phase_deg):
    """20 log10 |K1 / K2|, K1 = (1 + g e^{-j phi}) / 2, K2 = (1 - g e^{j phi}) / 2"""
    g, phi = 10.0 ** (gain_db / 20.0), math.radians(phase_deg)
    k1, k2 = (1.0 + g * np.exp(-1j * phi)) / 2.0, (1.0 - g * np.exp(1j * phi)) / 2.0
    return 20.0 * math.log10(abs(k1) / abs(k2))


def impair(z, gain_db, phase_deg, dc=0j):
    """A proper complex signal z through the receiver's imbalance, in float: I = Re z, Q = g Im(e^{-j phi} z) = g (Im z cos phi
    - Re z sin phi) -- which is K1 z + K2 conj(z) --, plus dc"""
    g, phi = 10.0 ** (gain_db / 20.0), math.radians(phase_deg)
    z = np.asarray(z, np.complex128)
    return z.real + 1j * g * (z.imag * math.cos(phi) - z.real * math.sin(phi)) + dc


def quantise(z, fmt, full_scale=1.0):
    """complex float (|.| <= full_scale on each rail) -> flat interleaved samples of the format's dtype"""
    amp = {"cu8": 127.5, "ci8": 128.0, "ci16": 32768.0}[fmt]
    s = np.stack([z.real, z.imag], axis=1).reshape(-1) / full_scale * amp
    s = np.rint(s + 127.5) if fmt == "cu8" else np.rint(s)
    return np.clip(s, SAMPLE_MIN[fmt], SAMPLE_MAX[fmt]).astype(DTYPE[fmt])


# ---- the ghost scene: a strong emitter whose mirror image an unbalanced receiver turns into a detection ----------------------
GHOST_PAIRS = 1 << 19
GHOST_STRONG = (32, 0.18, 0.04)       # samples per symbol, centre, complex rms of full scale: about 40 dB above the floor per bin
GHOST_WEAK = (64, -0.33, 0.004)       # about 23 dB above the floor: its own image stays below it
GHOST_NOISE_RMS = 0.002
GHOST_IMBALANCE = (1.0, 5.0)          # dB, degrees: 22.83 dB of image rejection
GHOST_DC = 0.01 - 0.02j


def ghost_scene(seed=7, pairs=GHOST_PAIRS, imbalance=GHOST_IMBALANCE):
    """flat interleaved "ci16": two QPSK emitters with tests/signals.py's root-raised-cosine pulse and constellation, complex
    noise, then the receiver's imbalance and DC offset in float, then the quantiser"""
    import signals
    rng = np.random.default_rng(seed)
    n = np.arange(pairs)
    z = np.zeros(pairs, np.complex128)
    pts = signals._constellation("QPSK")
    for sps, fc, amp in (GHOST_STRONG, GHOST_WEAK):
        nsym = pairs // sps + 2
        up = np.zeros(nsym * sps, np.complex128)
        up[::sps] = pts[rng.integers(0, len(pts), nsym)]
        base = np.convolve(up, signals._rrc(sps), mode="same")[:pairs]
        z += amp / np.sqrt(np.mean(np.abs(base) ** 2)) * base * np.exp(2j * np.pi * fc * n)
    z += GHOST_NOISE_RMS / np.sqrt(2.0) * (rng.standard_normal(pairs) + 1j * rng.standard_normal(pairs))
    return quantise(impair(z, imbalance[0], imbalance[1], GHOST_DC), "ci16")
