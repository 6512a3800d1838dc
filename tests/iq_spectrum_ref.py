"""float64 numpy restatement of mdc_iq_spectrogram (include/mdc.h, "power spectrogram"): the definition the tests hold the kernel
to.  Written from the header's text, not from the kernel: np.fft.fft on the exactly widened, windowed integers (int64 products,
asserted below 2^30, exact in float64).  Also the synthetic three-emitter band the scan tests share."""
import numpy as np

from iq_ddc_ref import DTYPE, FMT, SAMPLE_MAX, SAMPLE_MIN, widen      # noqa: F401  (the widening is mdc_iq_ddc's, word for word)

MIN_NFFT, MAX_NFFT, MAX_AVG = 64, 4096, 4096
U = 2.0 ** -24


def rows_count(pairs, nfft, hop, avg):
    segs = (pairs - nfft) // hop + 1 if pairs >= nfft else 0
    return segs // avg


def segment_powers(iq, fmt, nfft, window, scale, starts):
    """P_s[k] = scale |X_s[k]|^2 for the segments starting at the listed pairs: (len(starts), nfft) float64."""
    I, Q = widen(iq, fmt)
    w = np.asarray(window).astype(np.int64)
    assert w.shape == (nfft,) and np.abs(w).max(initial=0) <= 32768
    idx = np.asarray(starts, np.int64)[:, None] + np.arange(nfft, dtype=np.int64)[None, :]
    vr, vi = I[idx] * w[None, :], Q[idx] * w[None, :]
    assert max(np.abs(vr).max(initial=0), np.abs(vi).max(initial=0)) < 2 ** 30
    X = np.fft.fft(vr.astype(np.float64) + 1j * vi.astype(np.float64), axis=1)
    return float(scale) * (X.real ** 2 + X.imag ** 2)


def spectrogram(iq, fmt, nfft, hop, avg, window, scale, rows=None):
    """(P, P_s, T_s): P[r,k] (rows, nfft), the per-segment scaled powers P_s (rows, avg, nfft) and their totals over the bins
    T_s (rows, avg) -- all float64.  rows: every row (None) or the listed row indices."""
    assert MIN_NFFT <= nfft <= MAX_NFFT and nfft & (nfft - 1) == 0 and hop >= 1 and 1 <= avg <= MAX_AVG
    pairs = np.asarray(iq).size // 2
    n_rows = rows_count(pairs, nfft, hop, avg)
    r = np.arange(n_rows, dtype=np.int64) if rows is None else np.asarray(rows, np.int64)
    assert r.size == 0 or (r.min() >= 0 and r.max() < n_rows)
    starts = ((r[:, None] * avg + np.arange(avg, dtype=np.int64)[None, :]) * hop).reshape(-1)
    Ps = segment_powers(iq, fmt, nfft, window, scale, starts).reshape(r.size, avg, nfft)
    return Ps.mean(axis=1), Ps, Ps.sum(axis=2)


def bound(P, Ps, Ts, nfft, avg):
    """The largest |P^ - P| the header allows, per row and bin: u = 2^-24, eps = 8u (log2 nfft + 1) -- Higham's bound for a
    power-of-two FFT in float32 with twiddle error <= 2u, plus the int -> f32 conversion -- gives every segment's spectrum within
    eps sqrt(T_s) of the exact one, so its power within 2 eps sqrt(P_s T_s) + eps^2 T_s; the squaring, the sum over avg segments
    and the final scaling add (avg + 4) u P."""
    eps = 8.0 * U * (np.log2(nfft) + 1.0)
    T = Ts[:, :, None]
    return (2.0 * eps * np.sqrt(Ps * T) + eps * eps * T).mean(axis=1) + (avg + 4) * U * P


# ---- the scan scenario: three QPSK emitters with a root-raised-cosine pulse in one "ci16" band -----------------------------
BAND_PAIRS = 1 << 18
BAND_SPS = (96, 48, 20)
BAND_CENTRES = (-0.31, 0.12, 0.36)
BAND_AMPLITUDES = (0.02, 0.05, 0.01)
BAND_NOISE_RMS = 0.002
BAND_DC = (0.01, -0.02)
RRC_BETA = 0.35


def rrc_pulse(sps, beta=RRC_BETA, span=12):
    """root-raised-cosine taps over `span` symbols each side, unit energy"""
    t = np.arange(-span * sps, span * sps + 1, dtype=np.float64) / sps
    with np.errstate(divide="ignore", invalid="ignore"):
        h = (np.sin(np.pi * t * (1 - beta)) + 4 * beta * t * np.cos(np.pi * t * (1 + beta))) / (np.pi * t * (1 - (4 * beta * t) ** 2))
    h[t == 0] = 1 - beta + 4 * beta / np.pi
    sing = np.isclose(np.abs(t), 1 / (4 * beta))
    h[sing] = beta / np.sqrt(2) * ((1 + 2 / np.pi) * np.sin(np.pi / (4 * beta)) + (1 - 2 / np.pi) * np.cos(np.pi / (4 * beta)))
    return h / np.sqrt((h * h).sum())


def synthetic_band(seed, pairs=BAND_PAIRS, emitters=True, noise=True, dc=True):
    """flat interleaved int16: the emitters (complex rms = amplitude x 32768 each), complex noise of rms 0.002 (both components
    together) and a DC offset of (0.01, -0.02) of full scale"""
    rng = np.random.default_rng(seed)
    n = np.arange(pairs)
    z = np.zeros(pairs, complex)
    if emitters:
        for sps, fc, amp in zip(BAND_SPS, BAND_CENTRES, BAND_AMPLITUDES):
            nsym = pairs // sps + 2
            sym = (rng.choice([-1.0, 1.0], nsym) + 1j * rng.choice([-1.0, 1.0], nsym)) / np.sqrt(2.0)
            up = np.zeros(nsym * sps, complex)
            up[::sps] = sym
            base = np.convolve(up, rrc_pulse(sps), mode="same")[:pairs]
            base *= amp / np.sqrt(np.mean(np.abs(base) ** 2))
            z += base * np.exp(2j * np.pi * fc * n)
    if noise:
        z += BAND_NOISE_RMS / np.sqrt(2.0) * (rng.standard_normal(pairs) + 1j * rng.standard_normal(pairs))
    if dc:
        z += BAND_DC[0] + 1j * BAND_DC[1]
    v = np.stack([z.real, z.imag], axis=1) * 32768.0
    return np.clip(np.rint(v), -32768, 32767).astype(np.dtype("<i2")).reshape(-1)


def band_psd(iq, nfft, window, scale):
    """all rows of the hop = nfft/2 spectrogram averaged: (nfft,) float64"""
    pairs = iq.size // 2
    segs = (pairs - nfft) // (nfft // 2) + 1
    acc = np.zeros(nfft)
    for s0 in range(0, segs, 256):
        starts = np.arange(s0, min(segs, s0 + 256), dtype=np.int64) * (nfft // 2)
        acc += segment_powers(iq, "ci16", nfft, window, scale, starts).sum(axis=0)
    return acc / segs
