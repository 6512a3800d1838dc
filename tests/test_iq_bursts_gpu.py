"""mdc_iq_spectrum_quantiles / frontend.spectrum_quantiles / VTCNN2.scan_iq(bursts=True) on the MI355X, against
tests/iq_quantile_ref.py:
  1. bit parity of the kernel with quantiles() over shapes around the kernel's row walk (1, 2, 3 rows: fewer than its 64 row
     lanes; 255 / 256 / 257: the tail loop around a multiple of them; 1000: the eight-rows-in-flight loop and its tail), rank
     lists and data families that make every radix pass alone decide;
  2. counts past 16 bits;
  3. determinism and graph capture (the ranks travel with the launch);
  4. on a real spectrogram through the package;
  5. the scan end to end: bursts, duty and gated labels are what the reference functions give from the device spectrogram;
  6. the example's --scan --bursts path."""
import ctypes
import functools
import gc
import importlib.util
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import iq_quantile_ref as Q                                                              # noqa: E402
from conftest import ROOT                                                                # noqa: E402
from modulationdetectioncnn_amd import VTCNN2, _cabi, frontend                           # noqa: E402

SENTINEL = 0xFFC0DEAD      # a NaN pattern no family below holds


def _run(P, ranks):
    """the kernel on the host matrix P (rows, nfft) float32: power_dev starts one float into a larger allocation; the output is
    pre-filled with a sentinel and has one guard row behind it, checked untouched.  Returns (nranks, nfft) uint32."""
    rows, nfft = P.shape
    buf = torch.empty(rows * nfft + 3, dtype=torch.float32, device="cuda")
    dev = buf[1:1 + rows * nfft]
    dev.copy_(torch.from_numpy(np.ascontiguousarray(P).reshape(-1)))
    out = torch.full(((len(ranks) + 1) * nfft,), SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
    r = np.asarray(ranks, np.int64)
    _cabi.check(_cabi.lib().mdc_iq_spectrum_quantiles(dev.data_ptr(), rows, nfft, r.ctypes.data, r.size, out.data_ptr(),
                                                      torch.cuda.current_stream().cuda_stream))
    got = out.cpu().numpy().view(np.uint32).reshape(len(ranks) + 1, nfft)
    assert (got[-1] == SENTINEL).all(), "the guard row behind the output was written"
    return got[:-1]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _families(rows, nfft, seed):
    """name -> (rows, nfft) float32"""
    rng = np.random.default_rng(seed)
    shape = (rows, nfft)
    noise = (rng.exponential(1.0, shape) * 1e-6).astype(np.float32)
    k = np.arange(nfft, dtype=np.float32)[None, :]
    fam = {"exponential": noise,
           "one value": np.broadcast_to((1.0 + k).astype(np.float32), shape).copy(),
           "two values": np.where(rng.random(shape) < 0.3, np.float32(2.5) + k, np.float32(0.125) * (1 + k)).astype(np.float32),
           "ascending": np.sort(noise, axis=0),
           "descending": np.sort(noise, axis=0)[::-1].copy(),
           "column offset": (noise * 1e6 + k).astype(np.float32)}
    base = np.uint32(0x3F4A2B1C)
    for b in range(4):      # only byte b differs from the common base: the pass of that byte alone decides
        digit = rng.integers(0, 0x7F if b == 3 else 0x100, shape).astype(np.uint32)
        fam[f"byte {b}"] = ((base & ~np.uint32(0xFF << (8 * b))) | (digit << np.uint32(8 * b))).view(np.float32)
    special = np.array([0x00000000, 0x00000001, 0x007FFFFF, 0x00800000, 0x3F800000, 0x42C80000, 0x7F7FFFFF, 0x7F800000], np.uint32)
    fam["zeros, subnormals, ordinary, inf"] = special[rng.integers(0, special.size, shape)].view(np.float32)
    return fam


def _rank_lists(rows):
    return [(0,), (rows - 1,), (0, rows // 2, rows - 1),
            (rows - 1, 0, rows // 2, rows // 3, rows - 1, 1 % rows, rows // 2, (2 * rows) // 3)]


# ---------------------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("nfft", [64, 256, 4096])
@pytest.mark.parametrize("rows", [1, 2, 3, 255, 256, 257, 1000])
def test_kernel_is_the_reference_bit_for_bit(nfft, rows):
    lists = _rank_lists(rows)
    every = [r for ranks in lists for r in ranks]
    for name, P in _families(rows, nfft, seed=rows * 7 + nfft).items():
        want = _bits(Q.quantiles(P, every))      # one sort per family, shared by the rank lists
        at = 0
        for ranks in lists:
            got = _run(P, ranks)
            np.testing.assert_array_equal(got, want[at:at + len(ranks)], err_msg=f"{name}, ranks {ranks}")
            at += len(ranks)


def test_negative_and_nan_patterns_follow_the_unsigned_order():
    rows, nfft = 300, 64
    rng = np.random.default_rng(5)
    P = rng.integers(0, 1 << 32, (rows, nfft), dtype=np.uint64).astype(np.uint32).view(np.float32)      # every pattern there is
    ranks = (0, 17, 150, 298, 299)
    np.testing.assert_array_equal(_run(P, ranks), _bits(Q.quantiles(P, ranks)))


# ---------------------------------------------------------------------------------------------------------------- 2. wide counts
def test_counts_past_sixteen_bits():
    rows, nfft = 70000, 64
    ranks = (0, 1, 65535, 65536, 69999)
    rng = np.random.default_rng(6)
    equal = np.broadcast_to((3.0 + np.arange(nfft)).astype(np.float32)[None, :], (rows, nfft)).copy()
    np.testing.assert_array_equal(_run(equal, ranks), _bits(Q.quantiles(equal, ranks)))
    one_smaller = equal.copy()
    one_smaller[rng.integers(0, rows, nfft), np.arange(nfft)] = np.float32(0.5)
    got = _run(one_smaller, ranks)
    np.testing.assert_array_equal(got, _bits(Q.quantiles(one_smaller, ranks)))
    assert (got[0] == _bits(np.float32(0.5))).all() and (got[1] == _bits(equal[0])).all()


# ---------------------------------------------------------------------------------------------------------------- 3. graphs
def test_determinism_and_graph_capture():
    rows, nfft = 777, 256
    fam = _families(rows, nfft, seed=9)
    P = fam["exponential"]
    ranks = (5, 776, 388)
    first, second = _run(P, ranks), _run(P, ranks)
    np.testing.assert_array_equal(first, second)
    np.testing.assert_array_equal(first, _bits(Q.quantiles(P, ranks)))

    L = _cabi.lib()
    dev = torch.from_numpy(P.copy()).cuda()
    out = torch.zeros((len(ranks), nfft), dtype=torch.float32, device="cuda")
    host_ranks = (ctypes.c_int64 * len(ranks))(*ranks)
    _cabi.check(L.mdc_iq_spectrum_quantiles(dev.data_ptr(), rows, nfft, ctypes.addressof(host_ranks), len(ranks), out.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream))      # warm: the code object
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        _cabi.check(L.mdc_iq_spectrum_quantiles(dev.data_ptr(), rows, nfft, ctypes.addressof(host_ranks), len(ranks), out.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream))
    ctypes.memset(ctypes.addressof(host_ranks), 0xFF, ctypes.sizeof(host_ranks))      # the ranks travelled with the launch:
    del host_ranks                                                                    # overwritten, then freed
    gc.collect()
    for name in ("two values", "column offset"):
        dev.copy_(torch.from_numpy(fam[name]).cuda())      # same buffer, new spectrogram
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_bits(out.cpu().numpy()), _bits(Q.quantiles(fam[name], ranks)), err_msg=name)


# ---------------------------------------------------------------------------------------------------------------- 4. real data
NFFT, AVG, HOLD, SEED = 1024, 2, 0.98, 2


@functools.lru_cache(maxsize=None)
def _band():
    return Q.bursty_band(SEED)      # shared: nobody writes to it


def test_quantiles_of_a_device_spectrogram():
    iq, _ = _band()
    spec = frontend.spectrogram(iq, "ci16", nfft=NFFT, avg=AVG)
    rows = spec.shape[0]
    assert rows == 255
    got = frontend.spectrum_quantiles(spec, (0.5, HOLD))
    assert got.shape == (2, NFFT) and got.dtype == torch.float32 and got.is_cuda
    want = Q.quantiles(spec.cpu().numpy(), [Q.rank_of(0.5, rows), Q.rank_of(HOLD, rows)])
    np.testing.assert_array_equal(_bits(got.cpu().numpy()), _bits(want))
    one = frontend.spectrum_quantiles(spec.cpu().numpy(), 1.0)      # a scalar q, a host array
    assert one.shape == (NFFT,) and torch.equal(one, spec.max(0).values)
    assert frontend.spectrum_quantiles(spec, ()).shape == (0, NFFT)


# ---------------------------------------------------------------------------------------------------------------- 5. end to end
def _by_hand(m, dev, e):
    """(plan, taps, probs, labels, dbfs) of one emitter: tune, resample, predict_iq -- the un-gated run"""
    shift, L, D, _ = frontend.channel_plan(e.centre, e.bandwidth)
    taps = frontend.plan_taps(L, D)
    down = frontend.ddc(dev, "ci16", shift=shift, decimate=D, taps=taps) if L == 1 else \
        frontend.resample(dev, "ci16", shift=shift, interpolate=L, decimate=D, taps=taps)
    down = down[:down.shape[0] // 128 * 128]
    return ((shift, L, D), taps) + tuple(m.predict_iq(down.reshape(-1), "ci16", normalize="rms", return_power=True))


def test_scan_iq_bursts_end_to_end():
    iq, truth = _band()
    m = VTCNN2.synthetic("deployed3")
    dev = torch.from_numpy(iq.copy()).cuda()
    records = m.scan_iq(dev, "ci16", nfft=NFFT, avg=AVG, bursts=True)
    w = frontend.design_window(NFFT)
    spec = frontend.spectrogram(dev, "ci16", nfft=NFFT, avg=AVG).cpu().numpy()      # the DEVICE spectrogram, on the host
    rows = spec.shape[0]
    q = Q.quantiles(spec, [Q.rank_of(0.5, rows), Q.rank_of(HOLD, rows)]).astype(np.float64)
    emitters = frontend.find_emitters(q[1], window=w)
    floor = float(np.median(q[0]))
    assert len(records) == len(emitters) == 4
    seen_burst = 0
    for rec, e in zip(records, emitters):
        assert (rec["centre"], rec["bandwidth"], rec["power_dbfs"], rec["snr_db"]) == tuple(e)
        first, count = Q.emitter_bins(e, NFFT)
        band = spec[:, (first + np.arange(count)) % NFFT].astype(np.float64).sum(axis=1)
        on_rows = Q.find_bursts(band, count * floor, 3.0, 1, 1)
        on = [Q.burst_pairs(a, z, NFFT, NFFT // 2, AVG) for a, z in on_rows]
        assert rec["bursts"] == on and rec["duty"] == sum(z - a for a, z in on_rows) / rows
        if abs(e.centre - Q.BURST_CENTRE) > 0.005:
            assert on == [(0, Q.burst_pairs(0, rows, NFFT, NFFT // 2, AVG)[1])] and rec["duty"] == 1.0      # never pauses
            continue
        seen_burst += 1
        assert len(on) == 2 and all(a < t1 and t0 < z for (a, z), (t0, t1) in zip(on, truth))      # both truth intervals, nothing else
        plan, taps, p, l, d = _by_hand(m, dev, e)
        assert (rec["shift"], rec["interpolate"], rec["decimate"]) == plan
        assert torch.equal(rec["probs"], p) and torch.equal(rec["window_dbfs"], d)      # untouched by the gate
        want = l.cpu().numpy().copy()
        for i in range(want.size):
            lo, hi = Q.window_support(i, 128, taps.size, plan[1], plan[2])
            if not any(a <= lo and hi < z for a, z in on):
                want[i] = -1
        got = rec["labels"].cpu().numpy()
        np.testing.assert_array_equal(got, want)
        assert (got >= 0).sum() >= 1 and (got < 0).sum() >= 1
        assert rec["label"] == int(np.bincount(got[got >= 0]).argmax())
    assert seen_burst == 1

    plain = m.scan_iq(dev, "ci16", nfft=NFFT, avg=AVG, bursts=False)      # the mean spectrum, as before
    mean = frontend.find_emitters(frontend.spectrogram(dev, "ci16", nfft=NFFT, avg=AVG).to(torch.float64).mean(0).cpu(), window=w)
    assert len(plain) == len(mean) >= 3
    for rec, e in zip(plain, mean):
        assert "bursts" not in rec and "duty" not in rec
        plan, _, p, l, d = _by_hand(m, dev, e)
        assert (rec["centre"], rec["bandwidth"]) == (e.centre, e.bandwidth) and (rec["shift"], rec["interpolate"], rec["decimate"]) == plan
        assert torch.equal(rec["probs"], p) and torch.equal(rec["labels"], l) and torch.equal(rec["window_dbfs"], d)
        open_ = l[l >= 0]
        assert rec["label"] == (int(torch.bincount(open_).argmax()) if open_.numel() else -1)
    m._release()


# ---------------------------------------------------------------------------------------------------------------- 6. the example
def test_example_scan_bursts_prints_four_rows(capsys):
    spec = importlib.util.spec_from_file_location("classify_capture", os.path.join(ROOT, "examples", "classify_capture.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    model = VTCNN2.synthetic("deployed3")
    found = ex.scan(model, ex.synthetic_band("ci16", bursty=True), "ci16", bursts=True)
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(found) == 4 and lines[0].startswith("4 emitters") and len(lines) == 2 + 4
    assert lines[1].split()[-2:] == ["bursts", "duty"]
    bursts = [int(line.split()[-2]) for line in lines[2:]]
    centres = [float(line.split()[0]) for line in lines[2:]]
    assert bursts == [1, 2, 1, 1] and abs(centres[1] + 0.08) < 0.005
    model._release()
