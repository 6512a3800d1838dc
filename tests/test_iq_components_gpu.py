"""mdc_iq_spectrogram_components / frontend.spectrogram_components / find_detections / VTCNN2.detect_iq on the MI355X, against
tests/iq_components_ref.py:
  1. bit parity of labels, count and records with components() over shapes around the kernels' tiles (32 x 64 cells) and chunks
     (1024 cells): one row, fewer rows than a tile, 33 and 257 rows (a tile and eight tiles plus one row), 64 columns (one
     tile wide) to 4096; every reach that takes another path (none, rows only, bins only, both, the largest); mask families that
     make the deepest trees, the most components, the most border crossings;
  2. what is off: equality, NaN, +Inf thresholds; the tie rule of the peak; the band's two ends and bin 0's two neighbours;
  3. capacity smaller than count, capacity 0 without a record buffer;
  4. determinism and graph capture;
  5. the detector end to end through the package, VTCNN2.detect_iq against the chain by hand, and the example."""
import functools
import importlib.util
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import iq_components_ref as R                                                            # noqa: E402
from conftest import ROOT                                                                # noqa: E402
from modulationdetectioncnn_amd import VTCNN2, _cabi, frontend                           # noqa: E402
from modulationdetectioncnn_amd.frontend import detection_threshold, find_detections, spectrogram_components  # noqa: E402,F401

SENTINEL = -559038737      # 0xDEADBEEF as int32: no label
REACHES = [(0, 0), (1, 1), (0, 3), (4, 0), (2, 3), (4, 4)]


class _Buffers:
    """device buffers of one call, each with a guard behind it that must come back untouched; power starts one float into its
    allocation (4-byte alignment is all the ABI asks)"""

    def __init__(self, rows, nfft, capacity):
        cells = rows * nfft
        self.rows, self.nfft, self.capacity = rows, nfft, capacity
        self.power = torch.empty(cells + 3, dtype=torch.float32, device="cuda")
        self.thresh = torch.empty(nfft + 1, dtype=torch.float32, device="cuda")
        self.labels = torch.empty(cells + nfft, dtype=torch.int32, device="cuda")
        self.comps = torch.empty((capacity + 1, 4), dtype=torch.int64, device="cuda")
        self.count = torch.empty(2, dtype=torch.int64, device="cuda")
        self.ws_bytes = _cabi.check(_cabi.lib().mdc_iq_spectrogram_components_workspace(rows, nfft))
        self.work = torch.empty(self.ws_bytes // 8 + 2 + 8, dtype=torch.int64, device="cuda")
        self.work_at = (-self.work.data_ptr()) % 16 // 8
        self.poison()

    def poison(self):
        self.labels.fill_(SENTINEL)
        self.comps.fill_(0x5A5A5A5A5A5A5A5A)
        self.count.fill_(-7)
        self.work.fill_(0x3C3C3C3C3C3C3C3C)

    def load(self, P, thresh):
        self.power[1:1 + P.size].copy_(torch.from_numpy(np.ascontiguousarray(P).reshape(-1)))
        self.thresh[1:].copy_(torch.from_numpy(np.ascontiguousarray(thresh)))

    def call(self, a, b):
        _cabi.check(_cabi.lib().mdc_iq_spectrogram_components(
            self.power.data_ptr() + 4, self.rows, self.nfft, self.thresh.data_ptr() + 4, a, b, self.labels.data_ptr(),
            self.comps.data_ptr() if self.capacity else None, self.capacity, self.count.data_ptr(), self.work.data_ptr() + 8 * self.work_at,
            torch.cuda.current_stream().cuda_stream))

    def results(self):
        cells = self.rows * self.nfft
        labels = self.labels.cpu().numpy()
        assert (labels[cells:] == SENTINEL).all(), "the guard row behind the labels was written"
        count = self.count.cpu().numpy()
        assert count[1] == -7, "the word behind the count was written"
        comps = self.comps.cpu().numpy()
        n = min(int(count[0]), self.capacity)
        assert (comps[n:] == 0x5A5A5A5A5A5A5A5A).all(), "a record at or beyond min(count, capacity) was written"
        work = self.work.cpu().numpy()
        assert (work[:self.work_at] == 0x3C3C3C3C3C3C3C3C).all() and (work[self.work_at + self.ws_bytes // 8:] == 0x3C3C3C3C3C3C3C3C).all(), \
            "the workspace was written outside its bytes"
        return labels[:cells].reshape(self.rows, self.nfft), comps[:n].view(_cabi.IQ_COMPONENT).reshape(-1), int(count[0])


def _run(P, thresh, a, b, capacity):
    buf = _Buffers(P.shape[0], P.shape[1], capacity)
    buf.load(P, thresh)
    buf.call(a, b)
    return buf.results()


def _check(P, thresh, reach, what, capacity=None):
    want_labels, want_records, want_count = R.components(P, thresh, *reach)
    cap = want_count + 2 if capacity is None else capacity
    labels, records, count = _run(P, thresh, reach[0], reach[1], cap)
    assert count == want_count, f"{what}: count {count}, reference {want_count}"
    np.testing.assert_array_equal(labels, want_labels, err_msg=what)
    want_records = want_records[:min(want_count, cap)]
    for name in _cabi.IQ_COMPONENT.names:
        np.testing.assert_array_equal(records[name].view(np.int32), want_records[name].view(np.int32), err_msg=f"{what}: {name}")
    return count


def _power_of(mask_centred, rng, levels=None):
    """a centred boolean mask -> (P natural float32, thresh): on iff P > thresh, with a threshold that differs from bin to bin.
    levels: draw the on-cells' values from that many multiples of the threshold (equal peaks: the tie rule), else distinct ones"""
    rows, nfft = mask_centred.shape
    thresh = (1.0 + rng.random(nfft)).astype(np.float32)
    mask = np.roll(mask_centred, -(nfft // 2), axis=1)
    if levels:
        factor = (2.0 + rng.integers(0, levels, (rows, nfft))).astype(np.float32)
    else:
        factor = (1.5 + rng.random((rows, nfft))).astype(np.float32)
    off = rng.choice(np.array([0.0, 0.25, 1.0], np.float32), (rows, nfft))      # 1.0: equal to the threshold, off
    return np.where(mask, factor * thresh[None, :], off * thresh[None, :]).astype(np.float32), thresh


def _serpentine(rows, nfft, along_rows):
    m = np.zeros((rows, nfft), bool)
    if along_rows:      # every other row, joined at alternating ends: crosses every vertical tile border once per row
        m[0::2] = True
        for r in range(1, rows, 2):
            m[r, nfft - 1 if (r // 2) % 2 == 0 else 0] = True
    else:               # every other column, joined at the bottom and the top in turn: crosses the tiles' lower borders nfft / 2 times
        m[:, 0::2] = True
        for c in range(1, nfft, 2):
            m[rows - 1 if (c // 2) % 2 == 0 else 0, c] = True
    return m


def _stripes(n, reach):
    """positions along one axis whose steps cycle through reach, reach + 1, reach + 2: gaps of reach - 1, reach and reach + 1 cells"""
    at, pos, i = [], 0, 0
    while pos < n:
        at.append(pos)
        pos += max(1, reach + i % 3)
        i += 1
    sel = np.zeros(n, bool)
    sel[at] = True
    return sel


def _families(rows, nfft, reach, rng):
    """name -> centred mask"""
    r, c = np.mgrid[0:rows, 0:nfft]
    fam = {"empty": np.zeros((rows, nfft), bool), "full": np.ones((rows, nfft), bool), "checkerboard": (r + c) % 2 == 0}
    for density in (0.05, 0.3, 0.59):
        fam[f"random {density}"] = rng.random((rows, nfft)) < density
    sr, sc = _stripes(rows, reach[0]), _stripes(nfft, reach[1])
    fam["row stripes"] = np.broadcast_to(sr[:, None], (rows, nfft)).copy()
    fam["column stripes"] = np.broadcast_to(sc[None, :], (rows, nfft)).copy()
    fam["lattice"] = sr[:, None] & sc[None, :]
    ends = np.zeros((rows, nfft), bool)
    ends[:, 0] = ends[:, nfft - 1] = True                              # centred columns 0 and nfft - 1 of the same row: the band's two ends
    ends[rows // 2, :] = False
    fam["the two ends"] = ends
    zero = np.zeros((rows, nfft), bool)
    zero[::2, nfft // 2 - 1] = zero[::2, nfft // 2] = True             # natural bins nfft - 1 and 0: neighbours
    fam["around bin 0"] = zero
    if rows == 33 and nfft in (64, 256):
        fam["serpentine along rows"], fam["serpentine along columns"] = _serpentine(rows, nfft, True), _serpentine(rows, nfft, False)
    return fam


# ---------------------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("reach", REACHES)
@pytest.mark.parametrize("rows", [1, 2, 7, 33, 257])
@pytest.mark.parametrize("nfft", [64, 256, 4096])
def test_kernels_are_the_reference_bit_for_bit(nfft, rows, reach):
    rng = np.random.default_rng(nfft * 1000 + rows * 10 + reach[0] * 5 + reach[1])
    for name, mask in _families(rows, nfft, reach, rng).items():
        P, thresh = _power_of(mask, rng)
        count = _check(P, thresh, reach, f"{name}, {rows} x {nfft}, reach {reach}")
        if name == "empty":
            assert count == 0
        if name == "full":
            assert count == (rows * nfft if reach == (0, 0) else rows if reach[0] == 0 else nfft if reach[1] == 0 else 1)
        if name == "checkerboard" and reach == (1, 1):
            assert count == (1 if rows > 1 else nfft // 2)      # (one row: its on-cells are two columns apart)
        if name == "checkerboard" and reach == (0, 0):
            assert count == (rows * nfft + 1) // 2
        if name == "the two ends" and reach[0] == 0 and rows > 1:
            assert count == 2 * (rows - 1)      # they do not join across the band's edge
        if name == "around bin 0" and reach == (0, 3):
            assert count == (rows + 1) // 2     # natural bins nfft - 1 and 0 join


# ---------------------------------------------------------------------------------------------------------------- 2. values
@pytest.mark.parametrize("reach", [(1, 1), (2, 3)])
@pytest.mark.parametrize("rows,nfft", [(33, 64), (70, 256)])
def test_what_is_off_and_the_tie_rule_of_the_peak(rows, nfft, reach):
    rng = np.random.default_rng(rows + nfft + reach[1])
    mask = rng.random((rows, nfft)) < 0.35
    P, thresh = _power_of(mask, rng, levels=2)                                      # two values per bin: every component's peak is tied
    P[rng.random((rows, nfft)) < 0.05] = np.nan                                     # NaN power: off
    thresh[rng.choice(nfft, 5, replace=False)] = np.inf                             # +Inf thresholds: their bins are off
    thresh[[0, 1, nfft - 1]] = np.inf                                               # a DC guard
    P[rng.random((rows, nfft)) < 0.01] = np.inf                                     # +Inf power is on wherever the threshold is finite
    eq = rng.random((rows, nfft)) < 0.05
    P[eq] = np.broadcast_to(thresh[None, :], (rows, nfft))[eq]                      # equality (and +Inf == +Inf): off
    on = np.roll(R.centred_mask(P, thresh), -(nfft // 2), axis=1)
    assert not on[:, np.isinf(thresh)].any() and not on[np.isnan(P)].any() and not on[eq].any() and on[np.isinf(P) & np.isfinite(thresh)[None, :]].all()
    _check(P, thresh, reach, f"values, {rows} x {nfft}, reach {reach}")
    nan_thresh = thresh.copy()
    nan_thresh[5] = np.nan                                                          # a NaN on the threshold's side: off
    _check(P, nan_thresh, reach, "a NaN threshold")


def test_equal_peaks_go_to_the_smallest_centred_index():
    rows, nfft = 40, 64
    P = np.full((rows, nfft), 5.0, np.float32)       # one component, every cell the same pattern
    thresh = np.ones(nfft, np.float32)
    labels, records, count = _run(P, thresh, 1, 1, 4)
    assert count == 1 and (labels == 0).all()
    assert tuple(records[0]) == (0, rows, 0, nfft, rows * nfft, 5.0, 0, 0)      # centred column 0 = natural bin nfft / 2
    P[7, 3] = P[7, nfft // 2 + 2] = P[30, 1] = 6.0      # natural 3 is centred 35, natural nfft/2 + 2 is centred 2: row 7, centred column 2 wins
    _, records, _ = _run(P, thresh, 1, 1, 4)
    assert (records[0]["peak"], records[0]["peak_row"], records[0]["peak_bin"]) == (6.0, 7, 2)


# ---------------------------------------------------------------------------------------------------------------- 3. capacity
@pytest.mark.parametrize("rows,nfft", [(7, 64), (33, 256)])
def test_capacity_smaller_than_count_and_no_records_at_all(rows, nfft):
    rng = np.random.default_rng(rows)
    r, c = np.mgrid[0:rows, 0:nfft]
    P, thresh = _power_of((r + c) % 2 == 0, rng)
    total = (rows * nfft + 1) // 2
    for capacity in (rows * nfft + 5, total, total - 1, 100, 1, 0):      # (more records than cells; 0: comps_dev is NULL)
        assert _check(P, thresh, (0, 0), f"checkerboard, capacity {capacity}", capacity=capacity) == total
    assert _check(P, thresh, (1, 1), "checkerboard, one component, no records", capacity=0) == 1      # (rows > 1)


# ---------------------------------------------------------------------------------------------------------------- 4. graphs
def test_determinism_and_graph_replay():
    rows, nfft, reach = 257, 256, (2, 3)
    rng = np.random.default_rng(11)
    masks = [rng.random((rows, nfft)) < 0.06, _families(rows, nfft, reach, rng)["lattice"], rng.random((rows, nfft)) < 0.59]
    cases = [_power_of(m, rng, levels=3) for m in masks]
    want = [R.components(P, t, *reach) for P, t in cases]
    cap = max(w[2] for w in want) + 2
    first, second = _run(*cases[0], *reach, cap), _run(*cases[0], *reach, cap)
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes() if isinstance(a, np.ndarray) else a == b      # the same bits on a second run
    buf = _Buffers(rows, nfft, cap)
    buf.load(*cases[0])
    buf.call(*reach)                                   # warm: the code objects
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        buf.call(*reach)
    for (P, t), (want_labels, want_records, want_count) in zip(cases, want):
        buf.poison()                                   # the first results and the workspace are overwritten
        buf.load(P, t)                                 # the same buffers, a new spectrogram
        g.replay()
        torch.cuda.synchronize()
        labels, records, count = buf.results()
        assert count == want_count
        np.testing.assert_array_equal(labels, want_labels)
        assert records.tobytes() == want_records.view(_cabi.IQ_COMPONENT).tobytes()


# ---------------------------------------------------------------------------------------------------------------- 5. end to end
SEED = 1


@functools.lru_cache(maxsize=None)
def _band():
    return R.hopping_band(SEED)      # shared: nobody writes to it


def test_package_on_a_device_spectrogram():
    iq, truth = _band()
    spec = frontend.spectrogram(iq, "ci16", nfft=R.HOP_NFFT, avg=R.HOP_AVG)
    host = spec.cpu().numpy()
    for floor, db, guard in (("flat", 6.0, 1), ("per-bin", 4.0, 0)):
        thresh = frontend.detection_threshold(spec, db, guard, floor)
        assert thresh.shape == (R.HOP_NFFT,) and thresh.dtype == torch.float32 and thresh.is_cuda
        np.testing.assert_array_equal(thresh.cpu().numpy().view(np.uint32), R.detection_threshold(host, db, guard, floor).view(np.uint32))
    thresh = frontend.detection_threshold(spec)
    labels, records, count = frontend.spectrogram_components(spec, thresh, 2, 3)
    want_labels, want_records, want_count = R.components(host, thresh.cpu().numpy(), 2, 3)      # the reference on the DEVICE spectrogram
    assert labels.dtype == torch.int32 and labels.is_cuda and count == want_count and records.dtype == _cabi.IQ_COMPONENT
    np.testing.assert_array_equal(labels.cpu().numpy(), want_labels)
    assert records.tobytes() == want_records.tobytes()
    found = frontend.find_detections(spec, thresh, avg=R.HOP_AVG)
    want = frontend.detections_from_components(host, thresh.cpu().numpy(), want_records.view(_cabi.IQ_COMPONENT), want_count, avg=R.HOP_AVG)
    half = R.HOP_NFFT // 2
    assert found == want and len(found) == 8      # the dwell on bin 0 is two boxes at the defaults: the DC guard's gap of three is beyond reach_bins = 3
    assert found[2].stop_bin == half - 1 and found[3].first_bin == half + 2 and found[2].first_pair == found[3].first_pair
    open_thresh = frontend.detection_threshold(spec, dc_guard=0)      # only bin 0 off: the seven truth boxes, one of them across the centring seam
    seven = frontend.find_detections(spec, open_thresh, avg=R.HOP_AVG)
    l7, r7, c7 = R.components(host, open_thresh.cpu().numpy(), 2, 3)
    assert seven == frontend.detections_from_components(host, open_thresh.cpu().numpy(), r7.view(_cabi.IQ_COMPONENT), c7, avg=R.HOP_AVG) and len(seven) == 7
    assert seven[2].first_bin < half - 1 and seven[2].stop_bin > half + 2 and abs(seven[2].centre) * R.HOP_NFFT <= 2
    for d, (first_pair, stop_pair, centre, _) in zip(seven, truth):
        assert abs(d.centre - centre) * R.HOP_NFFT <= 2 and d.first_pair <= first_pair + 4096 and d.stop_pair >= stop_pair - 4096
    literal = R.find_detections(host, thresh.cpu().numpy(), want_records, want_count, avg=R.HOP_AVG)
    assert [tuple(d)[:5] + tuple(d)[9:] for d in found] == [w[:5] + w[9:] for w in literal]
    with pytest.raises(ValueError, match=f"{count} components, capacity is 3"):
        frontend.find_detections(spec, thresh, capacity=3)
    few = frontend.spectrogram_components(host, thresh.cpu().numpy(), 2, 3, capacity=3)      # host arrays are moved; labels are complete regardless
    assert few[2] == count and len(few[1]) == 3 and torch.equal(few[0], labels) and few[1].tobytes() == records[:3].tobytes()


def _by_hand(m, dev, d):
    """(plan, probs, labels, dbfs) of one detection: slice, tune, resample, predict_iq"""
    shift, L, D, _ = frontend.channel_plan(d.centre, d.bandwidth)
    taps = frontend.plan_taps(L, D)
    part = dev[2 * d.first_pair:2 * d.stop_pair]
    down = frontend.ddc(part, "ci16", shift=shift, decimate=D, taps=taps) if L == 1 else \
        frontend.resample(part, "ci16", shift=shift, interpolate=L, decimate=D, taps=taps)
    down = down[:down.shape[0] // 128 * 128]
    return ((shift, L, D),) + tuple(m.predict_iq(down.reshape(-1), "ci16", normalize="rms", return_power=True))


def test_detect_iq_is_the_chain_by_hand():
    iq, _ = _band()
    m = VTCNN2.synthetic("deployed3")
    dev = torch.from_numpy(iq.copy()).cuda()
    spec = frontend.spectrogram(dev, "ci16", nfft=1024, avg=8)
    records = m.detect_iq(dev, "ci16")                    # the defaults: the dwell on bin 0 is two boxes beside the DC guard
    found = frontend.find_detections(spec, frontend.detection_threshold(spec), avg=8)
    assert len(records) == len(found) == 8
    whole = m.detect_iq(dev, "ci16", dc_guard=0)          # seven, the third across the centring seam: planned with a centre next to 0
    found7 = frontend.find_detections(spec, frontend.detection_threshold(spec, dc_guard=0), avg=8)
    assert len(whole) == len(found7) == 7 and abs(whole[2]["centre"]) * 1024 <= 2 and abs(whole[2]["shift"]) * 1024 <= 2
    for rec, d in list(zip(records, found)) + list(zip(whole, found7)):
        assert tuple(rec[k] for k in d._fields) == tuple(d)
        plan, p, l, dbfs = _by_hand(m, dev, d)
        assert (rec["shift"], rec["interpolate"], rec["decimate"]) == plan
        assert torch.equal(rec["probs"], p) and torch.equal(rec["labels"], l) and torch.equal(rec["window_dbfs"], dbfs)
        assert rec["windows"] == l.shape[0] >= 1
        open_ = l[l >= 0]
        assert rec["label"] == (int(torch.bincount(open_).argmax()) if open_.numel() else -1)
    host = m.detect_iq(iq, "ci16")                                       # a numpy capture: numpy results, the same numbers
    assert [r["first_pair"] for r in host] == [r["first_pair"] for r in records]
    assert all(isinstance(r["labels"], np.ndarray) and np.array_equal(r["labels"], q["labels"].cpu().numpy()) for r, q in zip(host, records))
    # boxes too short for one window: windows 0, label -1, empty results
    short = m.detect_iq(dev[:2 * 8192], "ci16", nfft=64, avg=1, min_rows=1, min_bins=1, reach_rows=0, reach_bins=0, threshold_db=8.0)      # noise alone
    assert len(short) >= 1 and all(r["stop_pair"] - r["first_pair"] == 64 for r in short)
    assert all(r["windows"] == 0 and r["label"] == -1 and r["labels"].shape == (0,) and r["probs"].shape == (0, 3) for r in short)
    m._release()


def test_example_detections_prints_seven_rows(capsys):
    spec = importlib.util.spec_from_file_location("classify_capture", os.path.join(ROOT, "examples", "classify_capture.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    model = VTCNN2.synthetic("deployed3")
    found = ex.detections(model, ex.synthetic_hopper("ci16"), "ci16")
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(found) == 7 and lines[0].startswith("7 detections") and len(lines) == 2 + 7
    assert lines[1].split()[-1] == "label" and [int(line.split()[0]) for line in lines[2:]] == sorted(int(line.split()[0]) for line in lines[2:])
    model._release()
