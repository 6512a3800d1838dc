"""mdc_iq_extract / frontend.extract / VTCNN2.detect_iq(batched=True) on the MI355X: every job of a launch against the numpy int64
restatement of mdc_iq_resample (tests/iq_resample_ref.py) on the job's slice, bit for bit; the batched detector against the loop,
record for record.  The planner's host side: tests/test_iq_extract.py."""
import functools
import importlib.util
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import iq_components_ref as CR                                                           # noqa: E402
import iq_resample_ref as R                                                              # noqa: E402
from conftest import ROOT                                                                # noqa: E402
from modulationdetectioncnn_amd import VTCNN2, _cabi, frontend                           # noqa: E402

JOB = _cabi.IQ_EXTRACT_JOB
POISON, GUARD = 0x5A5A, 64


def _capture(fmt, pairs, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(R.SAMPLE_MIN[fmt], R.SAMPLE_MAX[fmt] + 1, size=2 * pairs).astype(R.DTYPE[fmt])


def _taps(n, seed, total=30000):
    """n int16 taps of both signs whose absolute values sum to at most `total`: within every branch's bound"""
    rng = np.random.default_rng(seed)
    h = rng.integers(-total // n, total // n + 1, size=n)
    return h.astype(np.int16)


def _out_count(pairs, ntaps, L, D):
    return R.out_count(pairs, ntaps, L, D)


def _run(iq, fmt, jobs, filters, gap=3):
    """One launch of jobs (first_pair, pairs, phase0, step, filter, n_out) laid out with `gap` untouched pairs in front of every
    job and a guard behind the last: (the output as (out_pairs + GUARD, 2) int16 numpy, the job records, out_pairs)"""
    rec = np.zeros(len(jobs), JOB)
    at = 0
    for k, (first, pairs, phase0, step, f, n_out) in enumerate(jobs):
        at += gap
        rec[k] = (first, pairs, at, n_out, phase0, step, f, 0)
        at += n_out
    blob, out_pairs = frontend.extract_plan(rec, filters, fmt, iq.size // 2, out_pairs=at + gap)
    big = torch.full((out_pairs + GUARD, 2), POISON, dtype=torch.int16, device="cuda")
    got = frontend.extract_run(iq, fmt, blob, out_pairs, out=big[:out_pairs])
    assert got.data_ptr() == big.data_ptr()
    return big.cpu().numpy(), rec, out_pairs


def _check(out, rec, out_pairs, iq, fmt, jobs, filters):
    """every job's range is the reference on its slice; everything else still holds the poison"""
    untouched = np.ones(out.shape[0], bool)
    for k, (first, pairs, phase0, step, f, n_out) in enumerate(jobs):
        L, D, h = filters[f]
        want = R.resample(iq[2 * first:2 * (first + pairs)], fmt, phase0, step, L, D, h)
        assert 0 <= n_out <= want.shape[0] == _out_count(pairs, h.size, L, D)
        a = int(rec["out_first"][k])
        np.testing.assert_array_equal(out[a:a + n_out], want[:n_out], err_msg=f"job {k}: L/D {L}/{D}, {h.size} taps, {fmt}")
        untouched[a:a + n_out] = False
    assert untouched[out_pairs:].all() and (out[untouched] == POISON).all()      # the gaps and the guard


# ---------------------------------------------------------------------------------------------------------------- 1. one mixed launch
PAIRS = 70001      # no multiple of 4: the capture's last quad is partial


@functools.lru_cache(maxsize=None)
def _mixed():
    filters = [(1, 1, np.array([32767], np.int16)),                  # 0: nothing but the mixer
               (1, 64, frontend.design_lowpass(64)),                  # 1: the DDC's case, 512 taps, even
               (2, 3, _taps(24, 1)),                                  # 2: an odd class; tile_out 5452
               (1, 2, _taps(16, 2)),                                  # 3: even: no output starts on an odd local sample
               (1, 256, _taps(1024, 3, 60000)),                       # 4: tiles of 28 outputs
               (32, 5, _taps(7, 4)),                                  # 5: fewer taps than branches: branches 7..31 are empty
               (3, 4, _taps(40, 5))]                                  # 6: odd (class 2 starts at local sample 3)
    near = frontend.phase_step(0.4999), frontend.phase_step(-0.4999)
    whole = lambda n: n // 128 * 128      # noqa: E731
    c = lambda j, f: _out_count(j, filters[f][2].size, *filters[f][:2])      # noqa: E731
    jobs = [(1, 5000, 0, 12345, 0, c(5000, 0)),                              # first_pair = 1 (mod 4)
            (2, 9000, 0xDEADBEEF, near[0], 1, whole(c(9000, 1))),             # = 2; trimmed to a frame; non-zero phase0
            (3, 20000, 77, near[1], 2, c(20000, 2)),                          # = 3; 13326 outputs in 3 tiles
            (10000, 9001, 0, 999999, 3, whole(c(9001, 3))),
            (20001, 40000, 1 << 31, 4242, 4, c(40000, 4)),                    # 153 outputs in 6 tiles
            (100, 600, 5, 1 << 29, 5, c(600, 5)),
            (40, 10, 0, 1, 2, 0),                                             # shorter than its filter: no output, no tile
            (PAIRS - 1000, 1000, 9, 31337, 6, c(1000, 6)),                    # ends on the capture's last pair
            (5000, 12000, 0, near[0], 2, whole(c(12000, 2))),                 # filter 2 again, not adjacent; reads what job 2 reads
            (2, 9000, 3, 70000, 1, c(9000, 1)),                               # filter 1 again, untrimmed; job 1's stretch
            (66000, 4001, 0, 0, 0, 4001)]                                     # ends on the last pair; whole-capture bound in a partial quad
    assert c(20000, 2) == 13326 and -(-13326 // 5452) == 3 and c(40000, 4) == 153 and c(10, 2) == 0 and jobs[1][5] == 128
    assert [j[0] % 4 for j in jobs[:3]] == [1, 2, 3] and jobs[10][0] + jobs[10][1] == PAIRS and PAIRS % 4
    return jobs, filters


@pytest.mark.parametrize("fmt", ["cu8", "ci8", "ci16"])
def test_every_job_is_the_resampler_on_its_slice(fmt):
    jobs, filters = _mixed()
    iq = _capture(fmt, PAIRS, 20)
    out, rec, out_pairs = _run(iq, fmt, jobs, filters)
    _check(out, rec, out_pairs, iq, fmt, jobs, filters)
    if fmt != "ci16":
        return
    dev = torch.from_numpy(iq).cuda()      # the package's own calls on the slices: the same bits once more
    for k in (1, 2, 9):
        first, pairs, phase0, step, f, n_out = jobs[k]
        L, D, h = filters[f]
        shift = ((step + (1 << 31)) % (1 << 32) - (1 << 31)) / 2.0 ** 32
        assert frontend.phase_step(shift) == step
        part = dev[2 * first:2 * (first + pairs)]
        a = int(rec["out_first"][k])
        res = frontend.resample(part, fmt, shift=shift, interpolate=L, decimate=D, taps=h, phase0=phase0).cpu().numpy()
        np.testing.assert_array_equal(out[a:a + n_out], res[:n_out])
        if L == 1:
            np.testing.assert_array_equal(frontend.ddc(part, fmt, shift=shift, decimate=D, taps=h, phase0=phase0).cpu().numpy(), res)


# ---------------------------------------------------------------------------------------------------------------- 2. more tiles than work-groups
def test_more_tiles_than_the_grid_cap():
    filters = [(1, 1, np.array([-32767], np.int16)), (2, 3, _taps(24, 6)), (1, 2, _taps(16, 7))]
    K = 1100
    iq = _capture("ci8", 150 * K + 300, 21)
    jobs = [(150 * k + (k % 3), 300 - (k % 7), k * 2654435761 % (1 << 32), k * 40503 % (1 << 32), k % 3,
             _out_count(300 - (k % 7), filters[k % 3][2].size, *filters[k % 3][:2])) for k in range(K)]
    assert all(j[5] > 0 for j in jobs) and K > _cabi.RESAMPLE_GRID_CAP      # one tile each: the kernel strides
    out, rec, out_pairs = _run(iq, "ci8", jobs, filters, gap=1)
    _check(out, rec, out_pairs, iq, "ci8", jobs, filters)


# ---------------------------------------------------------------------------------------------------------------- 3. the slice's end
@pytest.mark.parametrize("fmt", ["cu8", "ci16"])
def test_what_lies_beyond_a_job_does_not_leak_into_it(fmt):
    """the capture is full scale in front of the job's first pair and behind its last: the job's outputs are those of the slice"""
    filters = [(1, 3, _taps(21, 8)), (5, 3, _taps(33, 9)), (1, 1, np.array([32767], np.int16))]
    iq = _capture(fmt, 9000, 22)
    first, pairs = 1001, 5003
    iq[:2 * first] = R.SAMPLE_MAX[fmt]
    iq[2 * (first + pairs):] = R.SAMPLE_MAX[fmt]
    jobs = [(first, pairs, 11, 1 << 27, f, _out_count(pairs, filters[f][2].size, *filters[f][:2])) for f in range(3)]
    out, rec, out_pairs = _run(iq, fmt, jobs, filters)
    _check(out, rec, out_pairs, iq, fmt, jobs, filters)
    quiet = iq.copy()
    quiet[:2 * first] = quiet[2 * (first + pairs):] = 128 if fmt == "cu8" else 0
    np.testing.assert_array_equal(_run(quiet, fmt, jobs, filters)[0], out)      # what surrounds the job changes nothing


# ---------------------------------------------------------------------------------------------------------------- 4. graphs
def test_determinism_and_graph_replay():
    jobs, filters = _mixed()
    iq = _capture("ci16", PAIRS, 23)
    first, rec, out_pairs = _run(iq, "ci16", jobs, filters)
    second = _run(iq, "ci16", jobs, filters)[0]
    assert first.tobytes() == second.tobytes()
    blob, planned = frontend.extract_plan(rec, filters, "ci16", PAIRS, out_pairs=out_pairs)
    assert planned == out_pairs
    dev, plan_dev = torch.from_numpy(iq).cuda(), torch.from_numpy(blob).cuda()
    out = torch.full((out_pairs + GUARD, 2), POISON, dtype=torch.int16, device="cuda")
    L = _cabi.lib()

    def call(stream):
        _cabi.check(L.mdc_iq_extract(dev.data_ptr(), _cabi.IQ_CI16, PAIRS, blob.ctypes.data, plan_dev.data_ptr(), blob.size, out.data_ptr(), out_pairs,
                                     stream.cuda_stream))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):      # one stream, one kernel node: the call allocates and copies nothing
        call(side)
    torch.cuda.synchronize()
    other = _capture("ci16", PAIRS, 24)
    want = _run(other, "ci16", jobs, filters)[0]
    dev.copy_(torch.from_numpy(other))          # the same buffers, a new capture
    out.fill_(POISON)
    g.replay()
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == want.tobytes() != first.tobytes()


# ---------------------------------------------------------------------------------------------------------------- 5. the package
def test_extract_packs_whole_frames():
    iq = _capture("ci16", 30000, 25)
    h23, h1 = frontend.plan_taps(2, 3), frontend.plan_taps(1, 4)
    stretches = [(0, 9000, 0.1, 2, 3, h23), (9000, 9100, -0.2, 1, 4, h1), (500, 20500, -0.3, 1, 4, h1), (29000, 30000, 0.25, 2, 3, h23)]
    for whole in (True, False):
        block, offsets = frontend.extract(iq, "ci16", stretches, whole_frames=whole)
        assert block.is_cuda and block.dtype == torch.int16 and offsets.dtype == np.int64 and offsets[0] == 0 and block.shape == (offsets[-1], 2)
        got = block.cpu().numpy()
        for k, (a, z, shift, L, D, h) in enumerate(stretches):
            want = R.resample(iq[2 * a:2 * z], "ci16", 0, frontend.phase_step(shift), L, D, h)
            n = want.shape[0] // 128 * 128 if whole else want.shape[0]
            assert offsets[k + 1] - offsets[k] == n
            np.testing.assert_array_equal(got[offsets[k]:offsets[k + 1]], want[:n])
        assert (offsets[2] == offsets[1]) == whole      # the stretch of 100 pairs: 20 outputs, no frame
    block, offsets = frontend.extract(iq, "ci16", [])
    assert block.shape == (0, 2) and offsets.tolist() == [0]
    with pytest.raises(ValueError, match="does not lie inside the capture's 30000 pairs"):
        frontend.extract(iq, "ci16", [(0, 30001, 0.0, 1, 4, h1)])


@functools.lru_cache(maxsize=None)
def _band():
    return CR.hopping_band(1)      # shared: nobody writes to it


def _same_records(batched, loop, kind):
    assert len(batched) == len(loop)
    for b, r in zip(batched, loop):
        assert list(b) == list(r)      # key for key, in the same order
        for key in r:
            if key in ("probs", "labels", "window_dbfs"):
                assert isinstance(b[key], kind) and isinstance(r[key], kind) and b[key].dtype == r[key].dtype and b[key].shape == r[key].shape, key
                assert torch.equal(b[key], r[key]) if kind is torch.Tensor else b[key].tobytes() == r[key].tobytes(), key
            else:
                assert type(b[key]) is type(r[key]) and b[key] == r[key], key


def test_batched_detect_iq_gives_the_loops_records():
    iq, _ = _band()
    m = VTCNN2.synthetic("deployed3")
    dev = torch.from_numpy(iq.copy()).cuda()
    seven = m.detect_iq(dev, "ci16", dc_guard=0)
    assert len(seven) == 7 and all(r["windows"] >= 1 for r in seven) and any(r["label"] >= 0 for r in seven)
    _same_records(m.detect_iq(dev, "ci16", dc_guard=0, batched=True), seven, torch.Tensor)
    # a squelch at the median window's power: some windows of a detection open, some shut, some detections shut altogether or nearly
    median = float(torch.cat([r["window_dbfs"] for r in seven]).median())
    for kw in (dict(), dict(dc_guard=0, squelch_dbfs=median), dict(dc_guard=0, squelch_dbfs=0.0)):
        loop = m.detect_iq(dev, "ci16", **kw)
        _same_records(m.detect_iq(dev, "ci16", batched=True, **kw), loop, torch.Tensor)
        shut, windows = int(sum((r["labels"] < 0).sum() for r in loop)), sum(r["windows"] for r in loop)
        if "squelch_dbfs" not in kw:
            assert shut == 0 and len(loop) == 8      # the defaults: the dwell on bin 0 is two boxes beside the DC guard
        elif kw["squelch_dbfs"] == median:
            assert 0 < shut < windows
        else:
            assert shut == windows and all(r["label"] == -1 for r in loop)
    _same_records(m.detect_iq(iq, "ci16", dc_guard=0, batched=True), m.detect_iq(iq, "ci16", dc_guard=0), np.ndarray)      # a numpy capture
    # boxes too short for one window: windows 0, label -1, empty results
    kw = dict(nfft=64, avg=1, min_rows=1, min_bins=1, reach_rows=0, reach_bins=0, threshold_db=8.0)
    loop, batched = m.detect_iq(dev[:2 * 8192], "ci16", **kw), m.detect_iq(dev[:2 * 8192], "ci16", batched=True, **kw)
    assert len(loop) >= 1 and all(r["windows"] == 0 and r["label"] == -1 and r["probs"].shape == (0, 3) for r in batched)
    _same_records(batched, loop, torch.Tensor)
    assert m.detect_iq(dev, "ci16", threshold_db=90.0, batched=True) == [] == m.detect_iq(dev, "ci16", threshold_db=90.0)      # nothing found
    with pytest.raises(ValueError, match="batched=True needs hop == 128"):
        m.detect_iq(dev, "ci16", hop=64, batched=True)
    m._release()


def test_example_batched_prints_the_same_rows(capsys):
    spec = importlib.util.spec_from_file_location("classify_capture", os.path.join(ROOT, "examples", "classify_capture.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    model = VTCNN2.synthetic("deployed3")
    iq = ex.synthetic_hopper("ci16")
    ex.detections(model, iq, "ci16")
    loop = capsys.readouterr().out
    found = ex.detections(model, iq, "ci16", batched=True)
    batched = capsys.readouterr().out
    assert len(found) == 7 and batched == loop and len(loop.strip().splitlines()) == 2 + 7
    model._release()
