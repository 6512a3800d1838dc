"""numpy restatement of mdc_iq_spectrum_quantiles (include/mdc.h, "spectrum quantiles") and literal loop versions of the host
functions of the burst scan (frontend.find_bursts, burst_pairs, emitter_bins, window_support): the definitions the tests hold the
kernel and the package to.  Written from the header's and the docstrings' text, not from the code.  Also the synthetic band with
one intermittent emitter that the burst tests share."""
import numpy as np

import iq_spectrum_ref as S

MAX_RANKS = 8


def quantiles(P, ranks):
    """out[i][k]: the pattern at position ranks[i] of column k's 32-bit patterns sorted ascending as unsigned integers"""
    P = np.ascontiguousarray(P)
    assert P.dtype == np.float32 and P.ndim == 2 and P.shape[0] >= 1
    ranks = np.asarray(ranks, np.int64).reshape(-1)
    assert ranks.size == 0 or (ranks.min() >= 0 and ranks.max() < P.shape[0])      # (the limit of MAX_RANKS per call is the library's)
    return np.sort(P.view(np.uint32), axis=0)[ranks].view(np.float32)


def rank_of(q, rows):
    import math
    return math.floor(q * (rows - 1))


def find_bursts(band, floor, threshold_db=3.0, min_rows=1, merge_rows=1):
    """row by row: a run starts at an on-row, swallows gaps of at most merge_rows off-rows that an on-row follows, and is kept
    if it spans at least min_rows rows"""
    level = floor * 10.0 ** (threshold_db / 10.0)
    on = [float(b) > level for b in band]
    runs, r, n = [], 0, len(on)
    while r < n:
        if not on[r]:
            r += 1
            continue
        first = last = r
        r += 1
        while r < n:
            if on[r]:
                last = r
            elif r - last > merge_rows:
                break
            r += 1
        if last - first + 1 >= min_rows:
            runs.append((first, last + 1))
        r = last + 1
    return runs


def burst_pairs(first_row, stop_row, nfft, hop, avg):
    """every segment of every row, pair by pair: the smallest pair read and one past the largest"""
    lo = hi = None
    for r in range(first_row, stop_row):
        for s in range(r * avg, r * avg + avg):
            a, z = s * hop, s * hop + nfft - 1
            lo = a if lo is None else min(lo, a)
            hi = z if hi is None else max(hi, z)
    return lo, hi + 1


def emitter_bins(emitter, nfft):
    centre, bandwidth = float(emitter[0]), float(emitter[1])
    count = round(bandwidth * nfft)
    if count < 1:
        count = 1
    first = round(centre * nfft - (count - 1) / 2)
    while first < 0:
        first += nfft
    while first >= nfft:
        first -= nfft
    return first, count


def window_support(w, hop, ntaps, interpolate, decimate):
    """zero-stuffed, as iq_resample_ref.stuff does it: position p of the stuffed stream holds input pair p / L when L divides p
    and a zero otherwise; output j reads positions jD .. jD + T - 1.  The smallest and the largest input pair among the 128
    outputs of the window."""
    first = last = None
    for j in range(w * hop, w * hop + 128):
        p = np.arange(j * decimate, j * decimate + ntaps, dtype=np.int64)      # the stretch of the stuffed stream
        n = p[p % interpolate == 0] // interpolate                            # the input pairs it holds
        if n.size:
            first = int(n[0]) if first is None else min(first, int(n[0]))
            last = int(n[-1]) if last is None else max(last, int(n[-1]))
    return first, last


# ---- the burst scenario: iq_spectrum_ref.synthetic_band plus one QPSK emitter that is on 4.5 % of the time ------------------------
BURST_SPS, BURST_CENTRE, BURST_AMPLITUDE = 32, -0.08, 0.003
BURST_INTERVALS = ((0.40, 0.43), (0.80, 0.815))      # of the capture's P pairs, half-open


def bursty_band(seed, pairs=S.BAND_PAIRS):
    """(flat interleaved int16, truth): synthetic_band(seed) plus a root-raised-cosine QPSK emitter (beta 0.35, 32 samples per
    symbol, centre -0.08, complex rms 0.003 of full scale while it is on) that is on only during the pairs of truth, a list of
    half-open (first, stop) intervals"""
    base = S.synthetic_band(seed, pairs).astype(np.int64)
    rng = np.random.default_rng(seed + 100)      # a stream of its own: synthetic_band(seed) stays what it is
    nsym = pairs // BURST_SPS + 2
    sym = (rng.choice([-1.0, 1.0], nsym) + 1j * rng.choice([-1.0, 1.0], nsym)) / np.sqrt(2.0)
    up = np.zeros(nsym * BURST_SPS, complex)
    up[::BURST_SPS] = sym
    z = np.convolve(up, S.rrc_pulse(BURST_SPS), mode="same")[:pairs]
    z *= BURST_AMPLITUDE / np.sqrt(np.mean(np.abs(z) ** 2))
    z *= np.exp(2j * np.pi * BURST_CENTRE * np.arange(pairs))
    truth = [(int(a * pairs), int(b * pairs)) for a, b in BURST_INTERVALS]
    gate = np.zeros(pairs, bool)
    for a, b in truth:
        gate[a:b] = True
    z[~gate] = 0.0
    v = base + np.rint(np.stack([z.real, z.imag], axis=1) * 32768.0).astype(np.int64).reshape(-1)
    return np.clip(v, -32768, 32767).astype(np.dtype("<i2")), truth
