"""mdc_iq_extract's host side (include/mdc.h, "batched extraction"): the planner's validation, layout and determinism, the
package's filter dedupe, and frontend.segment_votes against a literal loop -- no GPU needed.  The kernel itself:
tests/test_iq_extract_gpu.py."""

import numpy as np
import pytest

from modulationdetectioncnn_amd import _cabi, frontend

EINVAL = -22
FILTER, JOB = _cabi.IQ_EXTRACT_FILTER, _cabi.IQ_EXTRACT_JOB


def _error():
    return _cabi.lib().mdc_last_error().decode()


def _records(jobs, filters):
    """jobs: (first_pair, pairs, out_first, n_out, phase0, step, filter[, reserved]); filters: (L, D, taps) -> the ABI's arrays"""
    taps = [np.asarray(f[2], np.int16) for f in filters]
    firsts = np.concatenate([[0], np.cumsum([t.size for t in taps])]).astype(int)
    frec = np.array([(L, D, t.size, int(a)) for (L, D, _), t, a in zip(filters, taps, firsts)], dtype=FILTER).reshape(-1)
    jrec = np.array([tuple(j) + (0,) * (8 - len(j)) for j in jobs], dtype=JOB).reshape(-1)
    return jrec, frec, np.ascontiguousarray(np.concatenate(taps)) if taps else np.zeros(0, np.int16)


def plan_bytes(jobs, filters):
    jrec, frec, _ = _records(jobs, filters)
    return int(_cabi.lib().mdc_iq_extract_plan_bytes(jrec.size, frec.size, jrec.ctypes.data, frec.ctypes.data))


def plan(jobs, filters, pairs_in, out_pairs, fmt=_cabi.IQ_CI16, nbytes=None):
    """(rc, blob) of mdc_iq_extract_plan; the blob's size is asked of mdc_iq_extract_plan_bytes unless given"""
    jrec, frec, h = _records(jobs, filters)
    L = _cabi.lib()
    if nbytes is None:
        nbytes = int(L.mdc_iq_extract_plan_bytes(jrec.size, frec.size, jrec.ctypes.data, frec.ctypes.data))
        assert nbytes > 0, _error()
    blob = np.full(nbytes, 0xA5, np.uint8)
    rc = L.mdc_iq_extract_plan(fmt, pairs_in, jrec.ctypes.data, jrec.size, frec.ctypes.data, frec.size, h.ctypes.data, h.size, out_pairs,
                               blob.ctypes.data, nbytes)
    return rc, blob


def tile_out(ntaps, L, D):
    """the documented geometry: ((8192 - ceil(T / L)) // D) * L outputs per tile"""
    return ((_cabi.RESAMPLE_TILE_PAIRS - -(-ntaps // L)) // D) * L


def out_count(pairs, ntaps, L, D):
    lv = (pairs - 1) * L + 1
    return (lv - ntaps) // D + 1 if pairs >= 1 and lv >= ntaps else 0


def header(blob):
    """the plan's header: magic, version, format, nfilters (int32) and njobs, ntiles, pairs_in, out_pairs, bytes (int64)"""
    return blob[:16].view(np.int32).tolist(), blob[16:56].view(np.int64).tolist()


def work_items(blob):
    """the plan's (job, tile) list: ntiles records of two int32 from the header's fourth offset on"""
    ntiles, at = int(blob[24:32].view(np.int64)[0]), int(blob[80:88].view(np.int64)[0])
    return blob[at:at + 8 * ntiles].view(np.int32).reshape(-1, 2)


ONE = np.array([32767], np.int16)
H24 = np.array([1365] * 24, np.int16)


def test_exports_and_record_sizes():
    for name in ("mdc_iq_extract", "mdc_iq_extract_plan", "mdc_iq_extract_plan_bytes"):
        assert name in _cabi.EXPORTS and hasattr(_cabi.lib(), name)
    assert FILTER.itemsize == 16 and JOB.itemsize == 48 and _cabi.lib().mdc_abi_version() == 5


def test_a_valid_plan_and_its_tile_count():
    filters = [(1, 1, ONE), (2, 3, H24), (1, 256, np.array([40] * 1024, np.int16)), (32, 5, np.array([100] * 7, np.int16))]
    stretches = [(0, 9000, 0), (100, 20000, 1), (7, 40000, 2), (50000, 3000, 3), (20, 10, 1), (60000, 20000, 1)]
    jobs, at, tiles = [], 0, 0
    for first, pairs, f in stretches:
        L, D, h = filters[f]
        n = out_count(pairs, h.size, L, D)
        jobs.append((first, pairs, at, n, 5, 77, f))
        at += n
        tiles += -(-n // tile_out(h.size, L, D))
    assert jobs[4][3] == 0 and -(-jobs[1][3] // 5452) == 3 and tile_out(24, 2, 3) == 5452 and tile_out(1024, 1, 256) == 28
    rc, blob = plan(jobs, filters, 80000, at)
    assert rc == 0, _error()
    (magic, version, fmt, nfilters), (njobs, ntiles, pairs_in, out_pairs, nbytes) = header(blob)
    assert (fmt, nfilters, njobs, pairs_in, out_pairs, nbytes) == (_cabi.IQ_CI16, 4, 6, 80000, at, blob.size)
    assert ntiles == tiles == 2 + 3 + 6 + 1 + 0 + 3
    assert blob.size % 16 == 0 and blob.size == plan_bytes(jobs, filters)
    # the work items: every (job, tile) once, the tiles of one filter adjacent
    items = work_items(blob)
    assert sorted(map(tuple, items.tolist())) == sorted((j, t) for j, job in enumerate(jobs) for t in range(-(-job[3] // tile_out(filters[job[6]][2].size, *filters[job[6]][:2]))))
    order = [jobs[j][6] for j, _ in items.tolist()]
    runs = [f for k, f in enumerate(order) if k == 0 or order[k - 1] != f]
    assert len(runs) == len(set(runs))      # each filter is one run of the list


def test_the_blob_is_deterministic():
    filters = [(2, 3, H24), (1, 4, np.arange(-8, 8).astype(np.int16))]
    jobs = [(0, 9000, 0, 128, 0, 1, 0), (50, 9000, 128, 256, 9, 1 << 31, 1), (3, 9000, 500, 5000, 0, 3, 0)]
    first, second = plan(jobs, filters, 10000, 6000), plan(jobs, filters, 10000, 6000)
    assert first[0] == second[0] == 0 and first[1].tobytes() == second[1].tobytes()
    other = plan(jobs[:2] + [(3, 9000, 500, 5000, 0, 4, 0)], filters, 10000, 6000)
    assert other[0] == 0 and other[1].tobytes() != first[1].tobytes()


def test_no_jobs_and_no_tiles():
    rc, blob = plan([], [], 100, 0)
    assert rc == 0 and header(blob)[1][:2] == [0, 0]
    rc, blob = plan([(0, 10, 0, 0, 0, 0, 0)], [(2, 3, H24)], 100, 0)      # a stretch shorter than its filter: no output, no tile
    assert rc == 0 and header(blob)[1][:2] == [1, 0]


CASES = [
    ([(0, 10, 0, 1, 0, 0, 0), (91, 10, 1, 1, 0, 0, 0)], [(1, 1, ONE)], 100, 2, "job 1: the stretch [91, 101) ends beyond the capture's 100 pairs"),
    ([(0, 100, 0, 34, 0, 0, 0)], [(1, 3, ONE)], 100, 34, None),                                       # out_count exactly
    ([(0, 100, 0, 35, 0, 0, 0)], [(1, 3, ONE)], 100, 35, "job 0: n_out is 35, its 100 pairs give at most 34 outputs"),
    ([(0, 100, 0, -1, 0, 0, 0)], [(1, 3, ONE)], 100, 35, "job 0: n_out is -1"),
    ([(0, 100, 0, 10, 0, 0, 0), (0, 100, 20, 10, 0, 0, 0), (0, 100, 10, 10, 0, 0, 0)], [(1, 1, ONE)], 100, 30, None),   # merely touching
    ([(0, 100, 0, 10, 0, 0, 0), (0, 100, 20, 10, 0, 0, 0), (0, 100, 9, 10, 0, 0, 0)], [(1, 1, ONE)], 100, 30,
     "job 2: its output range [9, 19) overlaps that of job 0, [0, 10)"),
    ([(0, 100, 0, 10, 0, 0, 0), (0, 100, 5, 0, 0, 0, 0)], [(1, 1, ONE)], 100, 10, None),               # an empty range overlaps nothing
    ([(0, 100, 25, 10, 0, 0, 0)], [(1, 1, ONE)], 100, 34, "job 0: the output range [25, 25 + 10) is not inside the 34 output pairs"),
    ([(0, 100, -1, 10, 0, 0, 0)], [(1, 1, ONE)], 100, 34, "job 0: the output range"),
    ([(0, 100, 0, 10, 0, 0, 0)], [(2, 1, np.array([32767, 1, 32767, 1, 1, 1], np.int16))], 100, 10, None),       # branch 0: 65535
    ([(0, 100, 0, 10, 0, 0, 0)], [(1, 1, ONE), (2, 1, np.array([1, 32767, 1, 32767, 1, 2], np.int16))], 100, 10,
     "filter 1: the absolute values of branch 1 of the taps (h[1], h[1 + 2], ...) sum to 65536"),
    ([(0, 100, 0, 10, 0, 0, 0, 7)], [(1, 1, ONE)], 100, 10, "job 0: reserved must be 0 (got 7)"),
    ([(0, 100, 0, 10, 0, 0, 0), (0, 100, 10, 10, 0, 0, 1)], [(1, 1, ONE)], 100, 20, "job 1: filter index 1 is not in 0..0"),
    ([(0, 100, 0, 10, 0, 0, -1)], [(1, 1, ONE)], 100, 20, "job 0: filter index -1"),
    ([(-1, 100, 0, 10, 0, 0, 0)], [(1, 1, ONE)], 100, 20, "job 0: first_pair and pairs must be in 0..2^58"),
    ([(0, 100, 0, 10, 0, 0, 0)], [(33, 1, ONE)], 100, 20, "filter 0: interpolate must be in 1..32 (got 33)"),
    ([(0, 100, 0, 10, 0, 0, 0)], [(1, 257, ONE)], 100, 20, "filter 0: decimate must be in 1..256 (got 257)"),
    ([(0, 100, 0, 1, 0, 0, 0)], [(1, 1, np.zeros(1025, np.int16))], 100, 20, "filter 0: ntaps must be in 1..1024 (got 1025)"),
]


@pytest.mark.parametrize("jobs, filters, pairs_in, out_pairs, message", CASES)
def test_the_planner_validates(jobs, filters, pairs_in, out_pairs, message):
    if message is None:
        rc, _ = plan(jobs, filters, pairs_in, out_pairs)
        assert rc == 0, _error()
        return
    sized = plan_bytes(jobs, filters)
    if sized < 0:      # what the size call can see, it rejects with the same words
        assert sized == EINVAL and "mdc_iq_extract_plan_bytes: " + message in _error(), _error()
    rc, blob = plan(jobs, filters, pairs_in, out_pairs, nbytes=max(sized, 4096))
    assert rc == EINVAL and "mdc_iq_extract_plan: " + message in _error(), _error()
    assert (blob == 0xA5).all()      # nothing is written on an error


def test_the_size_call_sees_jobs_and_filters_alone():
    """what needs the capture's length, the output's length or the taps is the planner's to reject"""
    seen = {"n_out", "reserved", "filter index", "first_pair", "interpolate", "decimate", "ntaps"}
    for jobs, filters, _, _, message in CASES:
        assert (plan_bytes(jobs, filters) < 0) == (message is not None and any(word in message for word in seen)), message


def test_the_planner_checks_its_other_arguments():
    jobs, filters = [(0, 100, 0, 10, 0, 0, 0)], [(1, 1, ONE)]
    assert plan(jobs, filters, 100, 10, fmt=3)[0] == EINVAL and "unknown sample format" in _error()
    good = plan_bytes(jobs, filters)
    assert plan(jobs, filters, 100, 10, nbytes=good + 16)[0] == EINVAL and f"plan_bytes is {good + 16}, mdc_iq_extract_plan_bytes gives {good}" in _error()
    jrec, frec, h = _records(jobs, filters)
    L = _cabi.lib()
    assert L.mdc_iq_extract_plan(2, 100, jrec.ctypes.data, 1, frec.ctypes.data, 1, h.ctypes.data, 1, 10, None, good) == EINVAL and "null plan" in _error()
    assert L.mdc_iq_extract_plan(2, 100, None, 1, frec.ctypes.data, 1, h.ctypes.data, 1, 10, None, good) == EINVAL and "null jobs" in _error()
    frec["first_tap"] = 1
    assert L.mdc_iq_extract_plan(2, 100, jrec.ctypes.data, 1, frec.ctypes.data, 1, h.ctypes.data, 1, 10, None, good) == EINVAL
    assert "filter 0: taps 1 .. 1 lie outside the 1 taps given" in _error()


def test_the_run_call_checks_the_plan_before_any_device_call():
    jobs, filters = [(0, 100, 0, 10, 0, 0, 0)], [(1, 1, ONE)]
    rc, blob = plan(jobs, filters, 100, 10)
    assert rc == 0
    L, p, n = _cabi.lib(), blob.ctypes.data, blob.size
    run = lambda *a: L.mdc_iq_extract(*a)      # noqa: E731
    assert run(None, 2, 100, None, None, n, None, 10, None) == EINVAL and "null plan" in _error()
    assert run(None, 2, 100, p, None, n - 16, None, 10, None) == EINVAL and f"plan_bytes is {n - 16}, the plan holds {n} bytes" in _error()
    assert run(None, 1, 100, p, None, n, None, 10, None) == EINVAL and "format is 1, the plan was made for 2" in _error()
    assert run(None, 2, 101, p, None, n, None, 10, None) == EINVAL and "pairs_in is 101, the plan was made for 100" in _error()
    assert run(None, 2, 100, p, None, n, None, 11, None) == EINVAL and "out_pairs is 11, the plan was made for 10" in _error()
    assert run(2, 2, 100, p, None, n, None, 10, None) == EINVAL and "whole (I,Q) pair" in _error()
    assert run(None, 2, 100, p, None, n, 2, 10, None) == EINVAL and "output must be 4-byte aligned" in _error()
    assert run(None, 2, 100, p, 4, n, None, 10, None) == EINVAL and "plan_dev must be 8-byte aligned" in _error()
    assert run(None, 2, 100, p, None, n, None, 10, None) == EINVAL and "null buffer" in _error()
    damaged = blob.copy()
    damaged[0] ^= 1
    assert run(None, 2, 100, damaged.ctypes.data, None, n, None, 10, None) == EINVAL and "does not hold a plan" in _error()
    rc, empty = plan([(0, 10, 0, 0, 0, 0, 0)], [(2, 3, H24)], 100, 0)      # no tile: MDC_OK without a launch, whatever the buffers
    assert rc == 0 and run(None, 2, 100, empty.ctypes.data, None, empty.size, None, 0, None) == 0


def test_extract_plan_dedupes_filters_and_packs_jobs():
    taps = np.arange(1, 25).astype(np.int16)
    filters = [(2, 3, taps), (1, 4, taps), (2, 3, taps.copy()), (2, 3, taps[::-1].copy()), (2, 3, taps.astype(np.int64))]
    jobs = [(0, 9000, 0, 1, k, 128 * (k + 1)) for k in range(5)]
    blob, out_pairs = frontend.extract_plan(jobs, filters, "ci16", 9000)
    (_, _, fmt, nfilters), (njobs, ntiles, pairs_in, planned, nbytes) = header(blob)
    assert (fmt, nfilters, njobs, ntiles, pairs_in, planned, nbytes) == (2, 3, 5, 5, 9000, out_pairs, blob.size) and out_pairs == 128 * 15
    rec = blob[96:96 + 48 * 5].view(JOB)
    assert rec["filter"].tolist() == [0, 1, 0, 2, 0] and rec["out_first"].tolist() == [0, 128, 384, 768, 1280]
    again, _ = frontend.extract_plan(jobs, filters, "ci16", 9000)
    assert again.tobytes() == blob.tobytes()
    # records as given: gaps stay gaps, and the planner's errors name the job
    given = np.array([(0, 9000, 10, 128, 0, 1, 1, 0), (0, 9000, 300, 128, 0, 1, 4, 0)], dtype=JOB)
    blob, out_pairs = frontend.extract_plan(given, filters, "cu8", 9000)
    assert out_pairs == 428 and blob[96:96 + 48 * 2].view(JOB)["filter"].tolist() == [1, 0] and header(blob)[0][2:] == [0, 3]
    assert frontend.extract_plan(given, filters, "cu8", 9000, out_pairs=500)[1] == 500
    given["filter"][1] = 5
    with pytest.raises(_cabi.MdcError, match="job 1: filter index -1"):
        frontend.extract_plan(given, filters, "cu8", 9000)
    with pytest.raises(_cabi.MdcError, match=r"job 0: the stretch \[0, 9000\) ends beyond the capture's 8999 pairs"):
        frontend.extract_plan(jobs, filters, "ci16", 8999)


def test_channel_plans_is_channel_plan_per_emitter():
    rng = np.random.default_rng(6)
    widths = [3 / 1024, 17 / 1024, 0.05, 0.16875, 0.2]
    emitters = [(float(rng.uniform(-0.5, 0.5)), widths[int(rng.integers(len(widths)))]) for _ in range(40)] + [(0.5, 0.05), (-0.5, 3 / 1024)]
    assert frontend.channel_plans(emitters) == [frontend.channel_plan(c, b) for c, b in emitters]
    assert frontend.channel_plans(emitters[:5], fill=0.3) == [frontend.channel_plan(c, b, 0.3) for c, b in emitters[:5]]
    assert frontend.channel_plans([]) == []
    for bad in ([(0.1, 0.05), (0.6, 0.05)], [(0.6, 0.05)], [(0.0, 0.05), (float("nan"), 0.05)]):
        with pytest.raises(ValueError, match="centre must lie in"):
            frontend.channel_plans(bad)


def _votes_literal(labels, offsets, classes):
    out = []
    for a, z in zip(offsets[:-1], offsets[1:]):
        counts = [sum(1 for v in labels[a:z] if v == c) for c in range(classes)]
        out.append(-1 if sum(counts) == 0 else counts.index(max(counts)))
    return out


def test_segment_votes_is_the_literal_loop():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(5)
    labels = rng.integers(-1, 4, size=400).astype(np.int32)
    labels[40:60] = -1                       # a segment of squelched windows alone
    labels[60:64] = [2, 1, 1, 2]             # ties go to the smallest class
    labels[64:70] = [3, 0, 3, 0, -1, -1]
    offsets = np.array([0, 40, 60, 64, 70, 70, 70, 199, 200, 400], np.int64)      # empty segments too
    want = _votes_literal(labels.tolist(), offsets.tolist(), 4)
    assert want[1] == -1 and want[2] == 1 and want[3] == 0 and want[4] == want[5] == -1
    for dtype in (torch.int32, torch.int64):
        got = frontend.segment_votes(torch.from_numpy(labels).to(dtype), offsets, 4)
        assert got.dtype == torch.int64 and got.tolist() == want
    assert frontend.segment_votes(torch.from_numpy(labels), torch.from_numpy(offsets), 4).tolist() == want
    # offsets that start late and stop early: windows outside every segment vote nowhere
    assert frontend.segment_votes(torch.from_numpy(labels), offsets[2:5], 4).tolist() == want[2:4]
    assert frontend.segment_votes(torch.from_numpy(labels[:0]), np.array([0, 0, 0]), 4).tolist() == [-1, -1]
    assert frontend.segment_votes(torch.from_numpy(labels), np.array([7]), 4).tolist() == []
    every = np.arange(401)                   # one window per segment: its own label
    assert frontend.segment_votes(torch.from_numpy(labels), every, 4).tolist() == labels.tolist()
