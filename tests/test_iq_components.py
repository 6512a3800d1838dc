"""The time-frequency detector without a GPU: mdc_iq_spectrogram_components' argument checks and workspace function, the Python
ValueErrors, the reference of tests/iq_components_ref.py against the header's text pair by pair and against scipy.ndimage.label,
the gap rule, frontend.detections_from_components against literal loops, and the claim the feature rests on, in numpy on the
reference spectrogram: a hopper's six dwells and a second emitter on an earlier dwell's bins come out as exactly seven boxes."""
import ctypes
import functools

import numpy as np
import pytest

import iq_components_ref as R
import iq_spectrum_ref as S
from modulationdetectioncnn_amd import _cabi, frontend
from modulationdetectioncnn_amd.frontend import detection_threshold, detections_from_components, find_detections, spectrogram_components  # noqa: F401

EINVAL = -22


# ------------------------------------------------------------------------------------------------------- 1. argument checks
def test_components_argument_checks_without_gpu():
    L = _cabi.lib()
    L.mdc_last_error.restype = ctypes.c_char_p
    buf = (ctypes.c_double * 4096)()                  # host memory is fine here: every check comes before any launch
    p = ctypes.addressof(buf)
    p += (-p) % 16

    def call(power=p, rows=4, nfft=64, thresh=p + 2048, a=1, b=1, labels=p + 4096, comps=p + 8192, capacity=4, count=p + 16384, work=p + 16400):
        return L.mdc_iq_spectrogram_components(power, rows, nfft, thresh, a, b, labels, comps, capacity, count, work, None)

    for kw in (dict(power=None), dict(thresh=None), dict(labels=None), dict(count=None), dict(work=None), dict(comps=None)):
        assert call(**kw) == EINVAL and b"null buffer" in L.mdc_last_error(), kw
    for nfft in (0, 32, 63, 96, 8192):
        assert call(nfft=nfft) == EINVAL and b"nfft" in L.mdc_last_error(), nfft
    for rows in (0, -1, 2 ** 31 // 64, 2 ** 40):      # rows * 64 == 2^31: one cell too many
        assert call(rows=rows) == EINVAL and b"rows" in L.mdc_last_error(), rows
    assert call(rows=2 ** 31 // 4096, nfft=4096) == EINVAL and b"rows" in L.mdc_last_error()
    for a in (-1, 5):
        assert call(a=a) == EINVAL and b"reach_rows" in L.mdc_last_error(), a
    for b in (-1, 5):
        assert call(b=b) == EINVAL and b"reach_bins" in L.mdc_last_error(), b
    assert call(capacity=-1) == EINVAL and b"capacity" in L.mdc_last_error()
    for name, off in (("power", 2), ("thresh", 2), ("labels", 2), ("comps", 4), ("count", 4), ("work", 8)):
        kw = {name: call.__defaults__[dict(power=0, thresh=3, labels=6, comps=7, count=9, work=10)[name]] + off}
        assert call(**kw) == EINVAL and (name + "_dev must be").encode() in L.mdc_last_error(), name
    assert _cabi.COMPONENTS_MAX_REACH == R.MAX_REACH == 4 and _cabi.COMPONENTS_MAX_CELLS == 2 ** 31 - 1 and _cabi.ABI_VERSION == 5
    assert _cabi.IQ_COMPONENT == R.COMPONENT and _cabi.IQ_COMPONENT.itemsize == 32
    assert "mdc_iq_spectrogram_components" in _cabi.EXPORTS and "mdc_iq_spectrogram_components_workspace" in _cabi.EXPORTS


def test_workspace_function_needs_no_device():
    L = _cabi.lib()
    for rows, nfft in ((1, 64), (16, 64), (17, 64), (257, 4096), (16384, 1024), (2 ** 31 // 64 - 1, 64)):
        chunks = -(-rows * nfft // _cabi.COMPONENTS_CHUNK)
        want = -(-chunks * 4 // 16) * 16
        assert L.mdc_iq_spectrogram_components_workspace(rows, nfft) == want == frontend.components_workspace(rows, nfft)
        assert want % 16 == 0 and want >= 16
    for rows, nfft in ((0, 64), (-3, 64), (4, 63), (4, 8192), (2 ** 31 // 64, 64), (2 ** 19, 4096)):
        assert L.mdc_iq_spectrogram_components_workspace(rows, nfft) == EINVAL, (rows, nfft)
    with pytest.raises(_cabi.MdcError):
        frontend.components_workspace(0, 64)


def test_python_errors_come_before_any_device():
    spec, thresh = np.zeros((5, 64), np.float32), np.zeros(64, np.float32)
    for shape in ((5,), (5, 96), (5, 32), (5, 8192), (2, 5, 64)):
        with pytest.raises(ValueError, match="spectrogram"):
            frontend.spectrogram_components(np.zeros(shape, np.float32), thresh)
    with pytest.raises(ValueError, match="no rows"):
        frontend.spectrogram_components(np.zeros((0, 64), np.float32), thresh)

    class Shape:      # only the shape is looked at before the cell limit: nothing that large is allocated
        shape = (2 ** 31 // 64, 64)

    with pytest.raises(ValueError, match="at most 2147483647 cells"):
        frontend.spectrogram_components(Shape(), thresh)
    for bad in (np.zeros(63, np.float32), np.zeros(65, np.float32), np.zeros((1, 64), np.float32)):
        with pytest.raises(ValueError, match="thresh must hold"):
            frontend.spectrogram_components(spec, bad)
    for kw in (dict(reach_rows=-1), dict(reach_rows=5), dict(reach_bins=-1), dict(reach_bins=5)):
        with pytest.raises(ValueError, match="reach"):
            frontend.spectrogram_components(spec, thresh, **kw)
    with pytest.raises(ValueError, match="capacity"):
        frontend.spectrogram_components(spec, thresh, capacity=-1)
    with pytest.raises(TypeError, match="spec must be float32"):
        frontend.spectrogram_components(spec.astype(np.float64), thresh)
    with pytest.raises(TypeError, match="thresh must be float32"):
        frontend.spectrogram_components(spec, thresh.astype(np.float64))
    with pytest.raises(ValueError, match="floor must be"):
        frontend.detection_threshold(spec, floor="median")
    with pytest.raises(ValueError, match="thresh must hold"):
        frontend.detections_from_components(spec, thresh[:63], np.zeros(0, _cabi.IQ_COMPONENT), 0)


# ------------------------------------------------------------------------------------------------------- 2. the reference itself
def _mask_to_power(mask_centred):
    """a centred boolean mask -> (P natural float32 with distinct values on the on-cells, thresh): on iff P > thresh"""
    rows, nfft = mask_centred.shape
    rng = np.random.default_rng(rows * 131 + nfft)
    vals = (2.0 + rng.random((rows, nfft))).astype(np.float32)
    Pc = np.where(mask_centred, vals, np.float32(0.5))
    return np.ascontiguousarray(np.roll(Pc, -(nfft // 2), axis=1)), np.ones(nfft, np.float32)


def _same_partition(labels_nat, other_centred, nfft):
    """our numbering (ascending root) from any labelling with 0 = off, 1.. = components"""
    mine = np.roll(labels_nat, nfft // 2, axis=1).reshape(-1)
    other = other_centred.reshape(-1)
    assert ((mine >= 0) == (other > 0)).all()
    on = np.flatnonzero(other > 0)
    _, first = np.unique(other[on], return_index=True)
    renumber = np.zeros(int(other.max()) + 1, np.int64)
    renumber[other[on][np.sort(first)]] = np.arange(first.size)      # components in order of their first cell
    np.testing.assert_array_equal(mine[on], renumber[other[on]])


@pytest.mark.parametrize("density", [0.05, 0.3, 0.6])
def test_reference_is_scipy_label_up_to_renumbering(density):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(int(density * 100))
    structures = {(1, 1): np.ones((3, 3), int), (0, 1): np.array([[0, 0, 0], [1, 1, 1], [0, 0, 0]]), (1, 0): np.array([[0, 1, 0], [0, 1, 0], [0, 1, 0]])}
    for rows, nfft in ((1, 64), (37, 64), (70, 256)):
        mask = rng.random((rows, nfft)) < density
        P, thresh = _mask_to_power(mask)
        for reach, structure in structures.items():
            labels, records, count = R.components(P, thresh, *reach)
            theirs, n = ndimage.label(mask, structure=structure)
            assert count == n == len(records)
            _same_partition(labels, theirs, nfft)
            boxes = ndimage.find_objects(theirs)
            sizes = np.bincount(theirs.reshape(-1))[1:]
            seen = set()
            for rec in records:      # every record is some scipy object's box and size, each used once
                r0, c0 = int(rec["row_first"]), int(rec["bin_first"])
                their = int(theirs[rec["peak_row"], rec["peak_bin"]])
                assert their > 0 and their not in seen
                seen.add(their)
                sl = boxes[their - 1]
                assert (sl[0].start, sl[0].stop, sl[1].start, sl[1].stop) == (r0, rec["row_stop"], c0, rec["bin_stop"])
                assert rec["cells"] == sizes[their - 1]
                inside = np.roll(P, nfft // 2, axis=1)[theirs == their]
                assert rec["peak"] == inside.max()


@pytest.mark.parametrize("reach", [(0, 0), (1, 1), (0, 3), (4, 0), (2, 3), (4, 4)])
def test_run_reference_is_the_literal_text(reach):
    rng = np.random.default_rng(sum(reach))
    for rows, nfft, density in ((1, 64, 0.5), (9, 64, 0.1), (33, 64, 0.3), (12, 128, 0.59)):
        P = rng.random((rows, nfft)).astype(np.float32)
        P[rng.random((rows, nfft)) < 0.02] = np.nan                     # NaN power is off
        P[0, :5] = np.float32(1.0 - density)                            # equality is off
        thresh = np.full(nfft, 1.0 - density, np.float32)
        thresh[[0, 1, nfft - 1]] = np.inf                               # a DC guard
        thresh[7] = np.nan                                              # a NaN threshold switches its bin off too
        a = R.components(P, thresh, *reach)
        b = R.components_literal(P, thresh, *reach)
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
        assert a[2] == b[2]
        on = R.centred_mask(P, thresh)
        assert not on[:, [nfft // 2 - 1, nfft // 2, nfft // 2 + 1, (7 + nfft // 2) % nfft]].any() and ((a[0] >= 0) == np.roll(on, -(nfft // 2), axis=1)).all()
        if reach == (0, 0):
            assert a[2] == int(on.sum()) and (a[1]["cells"] == 1).all()


@pytest.mark.parametrize("reach", [1, 2, 3, 4])
def test_a_gap_of_reach_minus_one_joins_and_gaps_of_reach_and_reach_plus_one_separate(reach):
    """a reach of g + 1 joins runs across g off cells: cells `reach` apart (a gap of reach - 1) are one component, cells
    `reach + 1` and `reach + 2` apart (gaps of exactly reach and reach + 1) are two"""
    rows, nfft = 12, 64
    for step, want in ((reach, 1), (reach + 1, 2), (reach + 2, 2)):
        for direction in ("rows", "bins", "both"):
            mask = np.zeros((rows, nfft), bool)
            mask[3, 20] = True
            mask[3 + (step if direction != "bins" else 0), 20 + (step if direction != "rows" else 0)] = True
            P, thresh = _mask_to_power(mask)
            labels, records, count = R.components(P, thresh, reach, reach)
            assert count == want, (reach, step, direction)
            assert R.components_literal(P, thresh, reach, reach)[2] == want
            if direction == "rows":      # the other direction's reach does not help
                assert R.components(P, thresh, 0, 4)[2] == 2 and R.components(P, thresh, reach, 0)[2] == want


def test_the_band_is_not_circular_and_bin_zero_has_two_neighbours():
    nfft = 64
    P = np.zeros((2, nfft), np.float32)
    thresh = np.ones(nfft, np.float32)
    P[0, nfft // 2 - 1] = P[0, nfft // 2] = 2.0       # natural bins nfft/2 - 1 and nfft/2: centred columns nfft - 1 and 0, the two ends
    P[1, nfft - 1] = P[1, 0] = 3.0                    # natural bins nfft - 1 and 0: centred columns nfft/2 - 1 and nfft/2, neighbours
    labels, records, count = R.components(P, thresh, 0, 1)
    assert count == 3
    assert labels[0, nfft // 2] == 0 and labels[0, nfft // 2 - 1] == 1 and labels[1, nfft - 1] == labels[1, 0] == 2
    assert tuple(records[2])[:5] == (1, 2, nfft // 2 - 1, nfft // 2 + 1, 2) and records[2]["peak_bin"] == nfft // 2 - 1      # equal peaks: the smaller index


# ------------------------------------------------------------------------------------------------------- 3. host half of find_detections
def test_detections_from_components_is_the_literal_loop():
    rng = np.random.default_rng(8)
    for rows, nfft in ((40, 64), (25, 256)):
        spec = rng.exponential(1.0, (rows, nfft)).astype(np.float32)
        for _ in range(6):      # a few blobs of different sizes in natural columns (one that wraps there lies at both ends of the band)
            r0, c0 = int(rng.integers(0, rows - 8)), int(rng.integers(0, nfft))
            h, w = int(rng.integers(1, 8)), int(rng.integers(1, 12))
            spec[r0:r0 + h, (c0 + np.arange(w)) % nfft] += np.float32(20.0)
        seam = (np.arange(nfft // 2 - 4, nfft // 2 + 5) + nfft // 2) % nfft      # centred columns nfft/2 - 4 .. nfft/2 + 4: natural -4 .. 4
        spec[rows - 7:rows - 2, seam] += (np.float32(20.0) + np.arange(9, dtype=np.float32))[None, :]      # lopsided: the centroid is off 0
        thresh = R.detection_threshold(spec, 6.0, -1, "flat")      # no DC guard: the blob on bin 0 stays whole
        for reach, min_rows, min_bins, hop, avg in (((1, 1), 3, 3, None, 1), ((2, 3), 1, 1, 48, 4), ((0, 0), 1, 1, None, 2), ((1, 2), 2, 5, nfft, 8)):
            _, records, count = R.components(spec, thresh, *reach)
            got = frontend.detections_from_components(spec, thresh, records.view(_cabi.IQ_COMPONENT), count, min_rows, min_bins, hop, avg)
            want = R.find_detections(spec, thresh, records, count, min_rows, min_bins, hop, avg)
            assert len(got) == len(want) and (reach != (0, 0) or len(got) == count)
            for g, w in zip(got, want):
                assert tuple(g)[:5] == w[:5] and tuple(g)[9:] == w[9:]
                np.testing.assert_allclose(tuple(g)[5:9], w[5:9], rtol=1e-12, atol=1e-15)      # float64 sums in another order
                assert g.stop_row - g.first_row >= min_rows and g.stop_bin - g.first_bin >= min_bins
            assert [(-0.5 <= g.centre < 0.5) for g in got] == [True] * len(got)
            assert got == sorted(got, key=lambda d: (d.first_pair, d.centre))
            if reach != (0, 0):      # the blob on bin 0 is one box across the centring seam (its centroid, across the wrap, is held to the loop's above)
                assert any(g.first_bin <= nfft // 2 - 4 and g.stop_bin >= nfft // 2 + 5 and g.first_row <= rows - 7 and g.stop_row >= rows - 2 for g in got), got
    assert frontend.detections_from_components(spec, thresh, records[:0], 0) == []


def test_detection_threshold_reference_levels():
    rng = np.random.default_rng(9)
    spec = rng.exponential(1.0, (21, 64)).astype(np.float32)
    flat = R.detection_threshold(spec, 6.0, 1, "flat")
    q0 = np.sort(spec, axis=0)[10]
    assert np.isinf(flat[[0, 1, 63]]).all() and (flat[2:63] == np.float32(np.sort(q0)[31]) * np.float32(10 ** 0.6)).all()
    per = R.detection_threshold(spec, 3.0, -1, "per-bin")
    np.testing.assert_array_equal(per, q0 * np.float32(10 ** 0.3))
    assert np.isinf(R.detection_threshold(np.zeros((5, 64), np.float32))).all()      # a floor that is not > 0


# ------------------------------------------------------------------------------------------------------- 4. the claim
SEEDS = (1, 2, 3)


@functools.lru_cache(maxsize=None)
def _case(seed):
    """(P float32 reference spectrogram, truth): computed once per seed, never written to"""
    iq, truth = R.hopping_band(seed)
    w = frontend.design_window(R.HOP_NFFT)
    P = S.spectrogram(iq, "ci16", R.HOP_NFFT, R.HOP_NFFT // 2, R.HOP_AVG, w, frontend.window_scale(w))[0].astype(np.float32)
    P.setflags(write=False)
    return P, truth


def _check_against_truth(found, truth, nfft, rows_pairs):
    """found and truth are both in order of (first_pair, centre): rows within +-1, centres within 2 bins, widths within a quarter"""
    assert len(found) == len(truth) == 7, found
    for d, (first_pair, stop_pair, centre, bandwidth) in zip(found, truth):
        assert abs(d.first_row - first_pair / rows_pairs) <= 1 and abs(d.stop_row - stop_pair / rows_pairs) <= 1, (d, first_pair, stop_pair)
        assert abs(d.centre - centre) * nfft <= 2, (d, centre)
        assert 0.75 * bandwidth <= d.bandwidth <= 1.25 * bandwidth, (d, bandwidth)
        assert d.first_pair == d.first_row * rows_pairs and d.stop_pair == (d.stop_row - 1) * rows_pairs + (R.HOP_AVG - 1) * (nfft // 2) + nfft


@pytest.mark.parametrize("seed", SEEDS)
def test_hopper_gives_its_seven_boxes_and_the_dc_guard_splits_the_dwell_on_bin_zero(seed):
    """The capture has no DC spike and its third dwell is centred on natural bin 0.  The defaults cannot give that dwell as one box:
    dc_guard = 1 switches centred columns nfft/2 - 1 .. nfft/2 + 1 off, a gap of three, and reach_bins = 3 bridges two.  So at the
    defaults the other six boxes are the truth's and the dwell on bin 0 is exactly two boxes, one on each side of the guard; with
    dc_guard = 0 (a gap of one) the seven truth boxes come out exactly, the one on bin 0 across the centring seam."""
    P, truth = _case(seed)
    nfft, rows_pairs, half = R.HOP_NFFT, R.HOP_AVG * R.HOP_NFFT // 2, R.HOP_NFFT // 2
    assert P.shape == (127, nfft) and len(truth) == 7 and truth[2][2] == 0.0

    thresh = R.detection_threshold(P)                                   # the defaults: 6 dB over the flat floor, DC guard 1
    _, records, count = R.components(P, thresh, 2, 3)                   # find_detections' default reach
    found = frontend.detections_from_components(P, thresh, records.view(_cabi.IQ_COMPONENT), count, avg=R.HOP_AVG)      # 3 x 3 at least
    assert len(found) == 8, found
    below, above = found[2], found[3]                                   # (the same first_pair; ordered by centre)
    assert below.stop_bin == half - 1 and above.first_bin == half + 2 and below.centre < 0.0 < above.centre
    assert abs(below.first_row - above.first_row) <= 1 and abs(below.stop_row - above.stop_row) <= 1
    assert abs((above.stop_bin - below.first_bin) / nfft - truth[2][3]) <= 0.25 * truth[2][3]      # together: the dwell's width
    merged = below._replace(first_row=min(below.first_row, above.first_row), stop_row=max(below.stop_row, above.stop_row),
                            stop_bin=above.stop_bin, centre=(below.centre + above.centre) / 2.0, bandwidth=(above.stop_bin - below.first_bin) / nfft)
    merged = merged._replace(first_pair=merged.first_row * rows_pairs,
                             stop_pair=(merged.stop_row - 1) * rows_pairs + (R.HOP_AVG - 1) * (nfft // 2) + nfft)
    _check_against_truth(found[:2] + [merged] + found[4:], truth, nfft, rows_pairs)

    thresh = R.detection_threshold(P, dc_guard=0)                       # only bin 0 itself is off
    _, records, count = R.components(P, thresh, 2, 3)
    found = frontend.detections_from_components(P, thresh, records.view(_cabi.IQ_COMPONENT), count, avg=R.HOP_AVG)
    _check_against_truth(found, truth, nfft, rows_pairs)
    across = found[2]
    assert across.first_bin < half - 1 and across.stop_bin > half + 2 and abs(across.centre) * nfft <= 2      # natural bins nfft-1 and 0 joined
    # the two emitters on the same bins (dwell 1 and the second emitter): two boxes, the same columns within 2, disjoint rows
    same = [d for d in found if abs(d.centre - R.HOP_CENTRES[R.HOP_SECOND[0]]) * nfft <= 2]
    assert len(same) == 2 and same[0].stop_row <= same[1].first_row and abs(same[0].first_bin - same[1].first_bin) <= 2
    # ... which one dimension at a time cannot tell apart: their bins hold ONE emitter in the quantile spectrum or in the mean
    emitters = frontend.find_emitters(P.astype(np.float64).mean(0))
    assert sum(abs(e.centre - R.HOP_CENTRES[R.HOP_SECOND[0]]) * nfft <= 2 for e in emitters) <= 1
