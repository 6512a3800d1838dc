"""Restatement of mdc_iq_spectrogram_components (include/mdc.h, "spectrogram components"): the definition the tests hold the
kernels and the package to.  Written from the header's text, not from the kernels.

`components_literal` is the text word for word -- every pair of on-cells inside the reach rectangle is united -- and is only fit
for small masks.  `components` is what the GPU tests compare with at a million cells: the same graph on ROW RUNS.  Within a row,
on-cells at most reach_bins apart are linked, so a row falls into runs (maximal chains of on-cells whose consecutive members are at
most reach_bins apart; a run may hold off cells); two runs [s1, e1] and [s2, e2] at most reach_rows rows apart hold a linked pair of
cells iff s2 <= e1 + reach_bins and s1 <= e2 + reach_bins (a cell of one run that falls into a gap of the other has a neighbour of
that gap within reach_bins).  The runs' graph is reduced with numpy (hook every edge's larger root under the smaller, then jump
pointers until flat; repeated until nothing moves).  tests/test_iq_components.py holds the two to each other and to
scipy.ndimage.label.

Also `hopping_band`, the synthetic hopper the detection tests share, and a literal-loop frontend.detections_from_components."""
import numpy as np

import iq_spectrum_ref as S

MAX_REACH = 4
COMPONENT = np.dtype([("row_first", np.int32), ("row_stop", np.int32), ("bin_first", np.int32), ("bin_stop", np.int32),
                      ("cells", np.int32), ("peak", np.float32), ("peak_row", np.int32), ("peak_bin", np.int32)])


def centred_mask(P, thresh):
    """on[r, c] for centred columns c = (k + nfft/2) mod nfft: power > threshold in float32; equality, NaN and +Inf thresholds off"""
    P = np.asarray(P)
    thresh = np.asarray(thresh)
    assert P.dtype == np.float32 and thresh.dtype == np.float32 and P.ndim == 2 and thresh.shape == (P.shape[1],)
    with np.errstate(invalid="ignore"):
        on = P > thresh[None, :]
    return np.roll(on, P.shape[1] // 2, axis=1)      # centred column c holds natural bin (c + nfft/2) mod nfft


def _finish(on, comp_of_cell, P, capacity):
    """comp_of_cell: for the on-cells in ascending r*nfft + c, any id that is equal exactly within a component -> (labels in
    natural positions, records, count) numbered by ascending root"""
    rows, nfft = on.shape
    idx = np.flatnonzero(on.reshape(-1)).astype(np.int64)
    labels_c = np.full(rows * nfft, -1, np.int32)
    if idx.size == 0:
        return np.roll(labels_c.reshape(rows, nfft), -(nfft // 2), axis=1), np.zeros(0, COMPONENT), 0
    uniq, first_at, inv = np.unique(comp_of_cell, return_index=True, return_inverse=True)      # first_at: a component's first cell = its root
    order = np.argsort(idx[first_at], kind="stable")
    number = np.empty(uniq.size, np.int64)
    number[order] = np.arange(uniq.size)
    lab = number[inv]
    labels_c[idx] = lab.astype(np.int32)
    count = int(uniq.size)
    r, c = idx // nfft, idx % nfft
    rec = np.zeros(count, COMPONENT)
    lo = np.full(count, np.iinfo(np.int64).max)
    for name, val, fn, start in (("row_first", r, np.minimum, lo), ("row_stop", r + 1, np.maximum, np.zeros(count, np.int64)),
                                 ("bin_first", c, np.minimum, lo), ("bin_stop", c + 1, np.maximum, np.zeros(count, np.int64))):
        acc = start.copy()
        fn.at(acc, lab, val)
        rec[name] = acc
    rec["cells"] = np.bincount(lab, minlength=count)
    Pc = np.roll(np.ascontiguousarray(P).view(np.uint32), nfft // 2, axis=1).reshape(-1)
    key = (Pc[idx].astype(np.uint64) << np.uint64(32)) | (~idx.astype(np.uint32)).astype(np.uint64)      # largest pattern, then smallest index
    best = np.zeros(count, np.uint64)
    np.maximum.at(best, lab, key)
    at = (~(best & np.uint64(0xFFFFFFFF)).astype(np.uint32)).astype(np.int64)
    rec["peak"] = (best >> np.uint64(32)).astype(np.uint32).view(np.float32)
    rec["peak_row"], rec["peak_bin"] = at // nfft, at % nfft
    labels = np.roll(labels_c.reshape(rows, nfft), -(nfft // 2), axis=1)      # back to natural positions
    return np.ascontiguousarray(labels), (rec if capacity is None else rec[:min(count, int(capacity))]), count


def components_literal(P, thresh, reach_rows, reach_bins, capacity=None):
    """the header's text, pair by pair (small masks only)"""
    on = centred_mask(P, thresh)
    rows, nfft = on.shape
    cells = [(int(r), int(c)) for r, c in zip(*np.nonzero(on))]
    parent = {rc: rc for rc in cells}

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    for (r, c) in cells:
        for r2 in range(r - reach_rows, r + reach_rows + 1):
            for c2 in range(c - reach_bins, c + reach_bins + 1):      # no wrap: the band is not circular
                if (r2, c2) in parent:
                    a, b = find((r, c)), find((r2, c2))
                    if a != b:
                        parent[max(a, b)] = min(a, b)
    comp = np.array([(lambda rc: rc[0] * nfft + rc[1])(find(rc)) for rc in cells], np.int64)
    return _finish(on, comp, P, capacity)


def components(P, thresh, reach_rows, reach_bins, capacity=None):
    """(labels int32 (rows, nfft) in natural positions, records (COMPONENT, trimmed to capacity), count)"""
    assert 0 <= reach_rows <= MAX_REACH and 0 <= reach_bins <= MAX_REACH
    on = centred_mask(P, thresh)
    rows, nfft = on.shape
    idx = np.flatnonzero(on.reshape(-1)).astype(np.int64)
    if idx.size == 0:
        return _finish(on, idx, P, capacity)
    r, c = idx // nfft, idx % nfft
    start = np.ones(idx.size, bool)
    start[1:] = (r[1:] != r[:-1]) | (c[1:] - c[:-1] > reach_bins)
    run_of = np.cumsum(start) - 1
    first = np.flatnonzero(start)
    last = np.r_[first[1:] - 1, idx.size - 1]
    row, s, e = r[first], c[first], c[last]
    n = row.size
    big = 2 * nfft + 16
    key_s, key_e = row * big + s, row * big + e      # ascending: runs are in (row, column) order and disjoint
    eu, ev = [], []
    for dr in range(1, reach_rows + 1):
        lo = np.searchsorted(key_e, (row + dr) * big + s - reach_bins, "left")       # first run of row + dr (or later) that ends at or after s - b
        hi = np.searchsorted(key_s, (row + dr) * big + e + reach_bins, "right")      # one past the last that starts at or before e + b
        cnt = np.maximum(hi - lo, 0)
        u = np.repeat(np.arange(n), cnt)
        v = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(lo, cnt)
        eu.append(u)
        ev.append(v)
    parent = np.arange(n)
    if eu:
        eu, ev = np.concatenate(eu), np.concatenate(ev)
        while eu.size:
            pu, pv = parent[eu], parent[ev]
            keep = pu != pv
            eu, ev, pu, pv = eu[keep], ev[keep], pu[keep], pv[keep]
            if eu.size == 0:
                break
            np.minimum.at(parent, np.maximum(pu, pv), np.minimum(pu, pv))
            while True:
                nxt = parent[parent]
                if np.array_equal(nxt, parent):
                    break
                parent = nxt
    return _finish(on, parent[run_of], P, capacity)


# ---- literal versions of the host functions of the detector ---------------------------------------------------------------------
def burst_pairs(first_row, stop_row, nfft, hop, avg):
    return first_row * avg * hop, ((stop_row - 1) * avg + avg - 1) * hop + nfft


def find_detections(spec, thresh, records, count, min_rows=3, min_bins=3, nfft_hop=None, avg=1):
    """frontend.detections_from_components in loops: tuples (first_row, stop_row, first_bin, stop_bin, cells, centre, bandwidth,
    peak_db, snr_db, first_pair, stop_pair) ordered by (first_pair, centre).  spec, thresh: host arrays in natural order."""
    spec = np.asarray(spec)
    thresh = np.asarray(thresh)
    rows, nfft = spec.shape
    hop = nfft // 2 if nfft_hop is None else nfft_hop
    out = []
    for i in range(min(count, len(records))):
        rec = records[i]
        r0, r1, c0, c1 = int(rec["row_first"]), int(rec["row_stop"]), int(rec["bin_first"]), int(rec["bin_stop"])
        if r1 - r0 < min_rows or c1 - c0 < min_bins:
            continue
        total = moment = 0.0
        for c in range(c0, c1):
            k = (c + nfft // 2) % nfft
            mean = 0.0
            for r in range(r0, r1):
                mean += float(spec[r, k])
            mean /= r1 - r0
            excess = mean - float(thresh[k]) if mean > float(thresh[k]) else 0.0
            total += excess
            moment += excess * ((c - nfft // 2) / nfft)
        centre = moment / total if total > 0.0 else ((c0 - nfft // 2) / nfft + (c1 - 1 - nfft // 2) / nfft) / 2.0
        peak = float(rec["peak"])
        at = float(thresh[(int(rec["peak_bin"]) + nfft // 2) % nfft])
        a, z = burst_pairs(r0, r1, nfft, hop, avg)
        out.append((r0, r1, c0, c1, int(rec["cells"]), centre, (c1 - c0) / nfft, 10.0 * np.log10(peak), 10.0 * np.log10(peak / at), a, z))
    out.sort(key=lambda d: (d[9], d[5]))
    return out


# ---- the hopper: six QPSK dwells, one after another, and a second emitter on an earlier dwell's bins ---------------------------------
HOP_NFFT, HOP_AVG = 1024, 8
HOP_PAIRS = 1 << 19
HOP_SPS = 32                                       # 1.35 / 32 of the band: about 43 bins of 1024
HOP_CENTRES = (-0.475, 0.21, 0.0, -0.18, 0.475, 0.33)      # 4 bins from either band edge; one centred on natural bin 0, across the centring seam
HOP_AMPLITUDE, HOP_NOISE_RMS = 0.002, 0.002      # about 14 dB per bin at nfft 1024
HOP_FIRST, HOP_DWELL, HOP_GAP = 1 << 14, 1 << 16, 1 << 13      # pairs: the first dwell's start, a dwell's length, the pause between dwells
HOP_SECOND = (1, 5)                                # the second emitter sits on dwell 1's centre during dwell 5's time


def hopping_band(seed, pairs=HOP_PAIRS):
    """(flat interleaved int16, truth): complex noise of rms 0.002, six root-raised-cosine QPSK dwells (32 samples per symbol,
    complex rms 0.002 while on) of 65,536 pairs each at HOP_CENTRES, 8,192 pairs apart, and one more emitter of the same kind on
    dwell 1's centre during dwell 5.  truth: seven (first_pair, stop_pair, centre, bandwidth) in order of (first_pair, centre);
    bandwidth is the pulse's occupied (1 + beta) / sps."""
    rng = np.random.default_rng(seed)
    n = np.arange(pairs)
    z = HOP_NOISE_RMS / np.sqrt(2.0) * (rng.standard_normal(pairs) + 1j * rng.standard_normal(pairs))
    spans = [(HOP_FIRST + i * (HOP_DWELL + HOP_GAP), HOP_FIRST + i * (HOP_DWELL + HOP_GAP) + HOP_DWELL) for i in range(len(HOP_CENTRES))]
    assert spans[-1][1] <= pairs
    plan = [(a, b, fc) for (a, b), fc in zip(spans, HOP_CENTRES)] + [(*spans[HOP_SECOND[1]], HOP_CENTRES[HOP_SECOND[0]])]
    for a, b, fc in plan:
        nsym = (b - a) // HOP_SPS + 2
        sym = (rng.choice([-1.0, 1.0], nsym) + 1j * rng.choice([-1.0, 1.0], nsym)) / np.sqrt(2.0)
        up = np.zeros(nsym * HOP_SPS, complex)
        up[::HOP_SPS] = sym
        base = np.convolve(up, S.rrc_pulse(HOP_SPS), mode="same")[:b - a]
        base *= HOP_AMPLITUDE / np.sqrt(np.mean(np.abs(base) ** 2))
        z[a:b] += base * np.exp(2j * np.pi * fc * n[a:b])
    v = np.stack([z.real, z.imag], axis=1) * 32768.0
    iq = np.clip(np.rint(v), -32768, 32767).astype(np.dtype("<i2")).reshape(-1)
    truth = sorted(((a, b, fc, (1.0 + S.RRC_BETA) / HOP_SPS) for a, b, fc in plan), key=lambda t: (t[0], t[2]))
    return iq, truth


def detection_threshold(P, threshold_db=6.0, dc_guard=1, floor="flat"):
    """frontend.detection_threshold on a host spectrogram: the lower median over time per bin, its lower median over the bins
    ("flat") or itself ("per-bin"), times 10^(threshold_db / 10) in float32; +inf within dc_guard of bin 0 and where the floor is
    not > 0"""
    P = np.asarray(P, np.float32)
    rows, nfft = P.shape
    q0 = np.sort(P.view(np.uint32), axis=0)[(rows - 1) // 2].view(np.float32)
    level = q0 if floor == "per-bin" else np.full(nfft, np.sort(q0)[(nfft - 1) // 2], np.float32)
    with np.errstate(invalid="ignore"):
        t = np.where(level > 0, level * np.float32(10.0 ** (threshold_db / 10.0)), np.float32(np.inf)).astype(np.float32)
    if dc_guard >= 0:
        t[np.arange(-dc_guard, dc_guard + 1) % nfft] = np.inf
    return t
