"""Restatement of mdc_iq_spectrogram_cfar (include/mdc.h, "spectrogram CFAR"): the definition the tests hold the kernel and the
package to.  Written from the header's text, not from the kernel: a loop over the cells, the training set as the cut-off window
minus the cut-off guard, np.partition on the uint32 view for the order statistic, one float32 division for the ratio, every NaN
of it stored as the one pattern the header names.

Also `cfar_brute`, a second, independent statement that sorts an explicit Python list of the training cells (small arrays only),
`cfar_threshold`, frontend.cfar_threshold on the host, and `motivating_scene`, the coloured spectrogram with a gain step that
shows what a local floor buys."""
import numpy as np

MAX_TRAIN_ROWS, MAX_TRAIN_BINS = 16, 128
NAN_PATTERN = np.uint32(0x7FC00000)      # what every NaN ratio is stored as


def _check(P, train_rows, train_bins, guard_rows, guard_bins, rank_permille):
    P = np.ascontiguousarray(P)
    assert P.dtype == np.float32 and P.ndim == 2 and P.shape[0] >= 1
    assert 0 <= guard_rows <= train_rows <= MAX_TRAIN_ROWS and 0 <= guard_bins <= train_bins <= MAX_TRAIN_BINS
    assert (train_rows, train_bins) != (guard_rows, guard_bins) and 0 <= rank_permille <= 1000
    return P


def cfar(P, train_rows=8, train_bins=32, guard_rows=2, guard_bins=8, rank_permille=500):
    """(floor, ratio): float32 (rows, nfft) in natural positions"""
    P = _check(P, train_rows, train_bins, guard_rows, guard_bins, rank_permille)
    rows, nfft = P.shape
    U = np.roll(P.view(np.uint32), nfft // 2, axis=1)      # centred column c holds natural bin (c + nfft/2) mod nfft
    F = np.empty((rows, nfft), np.uint32)
    for r in range(rows):
        r0, r1 = max(r - train_rows, 0), min(r + train_rows, rows - 1) + 1
        g0, g1 = max(r - guard_rows, 0), min(r + guard_rows, rows - 1) + 1
        for c in range(nfft):
            c0, c1 = max(c - train_bins, 0), min(c + train_bins, nfft - 1) + 1      # cut off: the band is not circular
            h0, h1 = max(c - guard_bins, 0), min(c + guard_bins, nfft - 1) + 1
            keep = np.ones((r1 - r0, c1 - c0), bool)
            keep[g0 - r0:g1 - r0, h0 - c0:h1 - c0] = False
            T = U[r0:r1, c0:c1][keep]
            n = T.size
            if n == 0:
                F[r, c] = 0x7F800000      # +Inf
            else:
                pos = ((n - 1) * rank_permille) // 1000
                F[r, c] = np.partition(T, pos)[pos]
    floor = np.ascontiguousarray(np.roll(F, -(nfft // 2), axis=1)).view(np.float32)      # back to natural positions
    with np.errstate(all="ignore"):
        ratio = (P / floor).astype(np.float32)      # float32 / float32: one correctly rounded division
    ratio.view(np.uint32)[np.isnan(ratio)] = NAN_PATTERN
    return floor, ratio


def cfar_brute(P, train_rows, train_bins, guard_rows, guard_bins, rank_permille):
    """the header's text cell by cell: an explicit list of the training cells' patterns, sorted (small arrays only)"""
    P = _check(P, train_rows, train_bins, guard_rows, guard_bins, rank_permille)
    rows, nfft = P.shape
    bits = P.view(np.uint32)
    floor = np.empty((rows, nfft), np.float32)
    for r in range(rows):
        for k in range(nfft):
            c = (k + nfft // 2) % nfft
            T = []
            for r2 in range(r - train_rows, r + train_rows + 1):
                for c2 in range(c - train_bins, c + train_bins + 1):
                    if not (0 <= r2 < rows and 0 <= c2 < nfft):
                        continue
                    if abs(r2 - r) <= guard_rows and abs(c2 - c) <= guard_bins:
                        continue
                    T.append(int(bits[r2, (c2 + nfft // 2) % nfft]))
            T.sort()
            pat = T[((len(T) - 1) * rank_permille) // 1000] if T else 0x7F800000
            floor[r, k] = np.array([pat], np.uint32).view(np.float32)[0]
    with np.errstate(all="ignore"):
        ratio = np.array([[np.float32(P[r, k]) / np.float32(floor[r, k]) for k in range(nfft)] for r in range(rows)], np.float32)
    for r in range(rows):
        for k in range(nfft):
            if ratio[r, k] != ratio[r, k]:
                ratio.view(np.uint32)[r, k] = 0x7FC00000
    return floor, ratio


def cfar_threshold(nfft, threshold_db=6.0, dc_guard=1):
    """frontend.cfar_threshold on the host: the float32 factor 10^(threshold_db / 10), +inf within dc_guard of bin 0"""
    t = np.full(nfft, np.float32(10.0 ** (threshold_db / 10.0)), np.float32)
    if dc_guard >= 0:
        t[np.arange(-dc_guard, dc_guard + 1) % nfft] = np.inf
    return t


# ---- the motivating case: a coloured front-end with a gain step -------------------------------------------------------------------
SCENE_ROWS, SCENE_NFFT, SCENE_AVG, SCENE_STEP_ROW = 96, 256, 8, 48
# (first row, stop row, first column, stop column), half-open, CENTRED columns: one continuous narrow emitter, a burst before the
# step, one after it, and one at the band's low end
SCENE_EMITTERS = ((0, 96, 40, 46), (10, 20, 200, 208), (60, 72, 100, 108), (30, 40, 20, 28))


def motivating_scene(seed=7):
    """(P, emitter): P, the (96, 256) float32 spectrogram in NATURAL positions -- chi-square noise of 2 * avg = 16 degrees of
    freedom (rng.chisquare(16) / 16), coloured by 10^(2 c / nfft) over the centred columns (20 dB across the band), times 10
    from row 48 on, and four emitters that each add floor * 10^1.2 times a fresh chi-square draw; emitter, the (96, 256) int
    array in CENTRED columns that holds -1 for a noise cell and i for a cell of emitter i."""
    rng = np.random.default_rng(seed)
    rows, nfft = SCENE_ROWS, SCENE_NFFT
    level = np.tile(10.0 ** (2.0 * np.arange(nfft) / nfft), (rows, 1))
    level[SCENE_STEP_ROW:] *= 10.0
    Pc = level * rng.chisquare(2 * SCENE_AVG, (rows, nfft)) / (2 * SCENE_AVG)
    emitter = np.full((rows, nfft), -1, np.int64)
    for i, (r0, r1, c0, c1) in enumerate(SCENE_EMITTERS):
        Pc[r0:r1, c0:c1] += level[r0:r1, c0:c1] * 10.0 ** 1.2 * rng.chisquare(2 * SCENE_AVG, (r1 - r0, c1 - c0)) / (2 * SCENE_AVG)
        emitter[r0:r1, c0:c1] = i
    return np.ascontiguousarray(np.roll(Pc, -(nfft // 2), axis=1)).astype(np.float32), emitter
