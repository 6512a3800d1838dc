"""mdc_iq_cf32_histogram / mdc_iq_cf32_quantize / frontend.quantize_cf32 on the MI355X.  The histogram is integer counts and the
quantiser one IEEE multiplication and one rounding per component, so every comparison is assert_array_equal against
tests/iq_cf32_ref.py (numpy, written from include/mdc.h):

  1. both kernels bit for bit: pairs in {1, 3, 255, 256, 257, 1023, 4099, 65541, grid cap x pairs per work-group + 1027} (every
     head and tail length; the last one reaches the stride loop), the buffer starting on a 16-byte boundary and 8 bytes after one;
     inputs: uniform random 32-bit patterns (every exponent, denormals, about 0.4 % non-finite values), Gaussian noise, and the
     edge list of the reference tiled; gains 2^-126, 2^-20, 1, 32768, 2^125 and 32768 / 0.7.  The histogram and the counts start
     from non-zero values (the calls ADD); the output is pre-filled with a sentinel, one guard pair after it untouched;
  2. two calls on two halves into the same histogram and counts equal the reference on the whole (the second half starts 8 bytes
     off a 16-byte boundary); counts_dev = NULL writes the same output;
  3. two runs give identical bits;
  4. round trips through frontend.quantize_cf32: integers with peak in [2^13, 2^14) times 2^-m come back exactly with the
     measured gain 2^m; any "ci16" capture / 32768 comes back exactly with full_scale=1.0, in every input form; scan_iq on that
     result equals scan_iq on the integer capture, key for key;
  5. non-finite pairs are zeroed and counted, or raise NonFiniteInputError with the count;
  6. examples/classify_capture.py's scan of the float copy of its own band lists the same emitters."""
import importlib.util
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import iq_cf32_ref as R                                                                   # noqa: E402
import signals                                                                            # noqa: E402
from conftest import ROOT                                                                 # noqa: E402
from modulationdetectioncnn_amd import NonFiniteInputError, VTCNN2, _cabi, frontend       # noqa: E402
from modulationdetectioncnn_amd import cf32_histogram, design_cf32_gain, quantize_cf32    # noqa: E402

BEYOND_CAP = _cabi.CF32_GRID_CAP * _cabi.CF32_GROUP_PAIRS + 1027
PAIRS = [1, 3, 255, 256, 257, 1023, 4099, 65541, BEYOND_CAP]
GAINS = [2.0 ** -126, 2.0 ** -20, 1.0, 32768.0, 2.0 ** 125, float(np.float32(32768 / 0.7))]
SENTINEL = 0x5A5A
HIST0 = np.arange(256, dtype=np.uint64) * 3 + 1
COUNTS0 = np.array([7, 1 << 40], np.uint64)


def _input(kind, pairs, seed):
    n = 2 * pairs
    rng = np.random.default_rng(seed)
    if kind == "bits":
        return rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32).view(np.float32)
    if kind == "gaussian":
        return (0.3 * rng.standard_normal(n)).astype(np.float32)
    return np.resize(R.EDGES, n)


def _on_device(x, lead):
    """x on the device, its first byte `lead` floats (0 or 2: 0 or 8 bytes) after a 16-byte boundary"""
    whole = torch.empty(x.size + 4, dtype=torch.float32, device="cuda")
    assert whole.data_ptr() % 16 == 0
    dev = whole[lead:lead + x.size]
    dev.copy_(torch.from_numpy(x.view(np.int32)).cuda().view(torch.float32))      # (as bits: no NaN is rewritten on the way)
    assert dev.data_ptr() % 16 == 4 * lead
    return dev


def _u64(a):
    return torch.from_numpy(np.asarray(a, np.uint64).view(np.int64).copy()).cuda()


def _histogram(dev, hist=None):
    """mdc_iq_cf32_histogram straight through the binding, into `hist` (int64 view of the uint64 counts; default: HIST0)"""
    hist = _u64(HIST0) if hist is None else hist
    _cabi.check(_cabi.lib().mdc_iq_cf32_histogram(dev.data_ptr(), dev.numel() // 2, hist.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return hist


def _quantize(dev, gain, counts="default"):
    """mdc_iq_cf32_quantize straight through the binding, with sentinel and guard pair; -> (int16 numpy, counts tensor or None)"""
    pairs = dev.numel() // 2
    out = torch.full((2 * pairs + 2,), SENTINEL, dtype=torch.int16, device="cuda")
    counts = _u64(COUNTS0) if isinstance(counts, str) else counts
    _cabi.check(_cabi.lib().mdc_iq_cf32_quantize(dev.data_ptr(), pairs, gain, out.data_ptr(), counts.data_ptr() if counts is not None else None,
                                                 torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert out[2 * pairs:].tolist() == [SENTINEL, SENTINEL]
    return out[:2 * pairs].cpu().numpy(), counts


def _host(t):
    return t.cpu().numpy().view(np.uint64)


# --------------------------------------------------------------------------------------------------------- 1. both kernels, bit for bit
@pytest.mark.parametrize("kind", ["bits", "gaussian", "edges"])
def test_kernels_bit_for_bit(kind):
    for i, pairs in enumerate(PAIRS):
        x = _input(kind, pairs, seed=100 + i)
        want_hist = HIST0 + R.histogram(x)
        want = [R.quantize(x, g) for g in GAINS]      # once per capture: the reference does not depend on where the buffer starts
        for lead in (0, 2):
            dev = _on_device(x, lead)
            np.testing.assert_array_equal(_host(_histogram(dev)), want_hist, err_msg=f"{kind} pairs={pairs} lead={lead}")
            for g, (ref_out, ref_bad, ref_clipped) in zip(GAINS, want):
                out, counts = _quantize(dev, g)
                msg = f"{kind} pairs={pairs} lead={lead} gain={g}"
                np.testing.assert_array_equal(out, ref_out, err_msg=msg)
                np.testing.assert_array_equal(_host(counts), COUNTS0 + np.array([ref_bad, ref_clipped], np.uint64), err_msg=msg)


def test_the_inputs_reach_what_they_are_there_for():
    h = R.histogram(_input("bits", 65541, 107))
    assert (h > 0).all() and 0.003 < h[255] / h.sum() < 0.005      # every exponent, denormals, about 0.4 % non-finite
    g = R.histogram(_input("gaussian", 65541, 107))
    assert np.sort(g)[-6:].sum() > 0.95 * g.sum()                   # concentrated: the histogram's contended case
    assert R.quantize(_input("edges", 7, 0), R.EDGE_GAIN)[2] == R.EDGES_CLIPPED


def test_output_aligned_to_one_pair_only():
    """out_dev wants 4 bytes, no more: whole quads leave as 16 bytes from any such address"""
    pairs = 4099
    x = _input("bits", pairs, 5)
    dev = _on_device(x, 2)
    ref = R.quantize(x, 32768.0)[0]
    for lead in (1, 2, 3):
        whole = torch.full((2 * (pairs + lead + 1),), SENTINEL, dtype=torch.int16, device="cuda")
        out = whole[2 * lead:]
        _cabi.check(_cabi.lib().mdc_iq_cf32_quantize(dev.data_ptr(), pairs, 32768.0, out.data_ptr(), None, torch.cuda.current_stream().cuda_stream))
        got = whole.cpu().numpy()
        np.testing.assert_array_equal(got[2 * lead:2 * (lead + pairs)], ref)
        assert (got[:2 * lead] == SENTINEL).all() and (got[2 * (lead + pairs):] == SENTINEL).all()


# ------------------------------------------------------------------------------------------------------------------ 2. accumulation
@pytest.mark.parametrize("kind", ["bits", "gaussian"])
def test_two_halves_accumulate_to_the_whole(kind):
    pairs, cut, gain = 65541, 30001, 32768.0      # the second half starts on an odd pair: 8 bytes off a 16-byte boundary
    x = _input(kind, pairs, 11)
    dev = _on_device(x, 0)
    a, b = dev[:2 * cut], dev[2 * cut:]
    assert b.data_ptr() % 16 == 8
    hist = _histogram(b, _histogram(a))
    np.testing.assert_array_equal(_host(hist), HIST0 + R.histogram(x))
    ref_out, ref_bad, ref_clipped = R.quantize(x, gain)
    out_a, counts = _quantize(a, gain)
    out_b, counts = _quantize(b, gain, counts)
    np.testing.assert_array_equal(np.concatenate([out_a, out_b]), ref_out)
    np.testing.assert_array_equal(_host(counts), COUNTS0 + np.array([ref_bad, ref_clipped], np.uint64))
    out, none = _quantize(dev, gain, None)      # counts_dev = NULL
    assert none is None
    np.testing.assert_array_equal(out, ref_out)


# --------------------------------------------------------------------------------------------------------------- 3. reproducibility
def test_two_runs_give_identical_bits():
    x = _input("bits", BEYOND_CAP, 21)
    dev = _on_device(x, 2)
    first = (_host(_histogram(dev)), *_quantize(dev, 32768.0))
    again = (_host(_histogram(dev)), *_quantize(dev, 32768.0))
    np.testing.assert_array_equal(first[0], again[0])
    np.testing.assert_array_equal(first[1], again[1])
    np.testing.assert_array_equal(_host(first[2]), _host(again[2]))


# -------------------------------------------------------------------------------------------------------------------- 4. round trips
def _integers_from_signals(peak=12000):
    """modulated frames of tests/signals.py as one interleaved stream of integers, the largest magnitude exactly `peak`"""
    frames, _, _ = signals.modulated_frames(64, seed=7)
    z = np.stack([frames[:, 0, :].reshape(-1), frames[:, 1, :].reshape(-1)], axis=1).reshape(-1).astype(np.float64)
    return np.rint(z / np.abs(z).max() * peak).astype(np.int16)


@pytest.mark.parametrize("m", [-3, 0, 14, 20, 100])
def test_integers_times_a_power_of_two_come_back_exactly(m):
    ints = _integers_from_signals()
    assert 2 ** 13 <= np.abs(ints.astype(np.int32)).max() < 2 ** 14
    x = (ints.astype(np.float64) * 2.0 ** -m).astype(np.float32)
    assert np.array_equal(x.astype(np.float64) * 2.0 ** m, ints)      # exact in float32
    out, rep = quantize_cf32(x, return_report=True)
    assert out.dtype == torch.int16 and out.is_cuda and out.shape == (ints.size,)
    assert rep == dict(gain=2.0 ** m, full_scale=32768.0 / 2.0 ** m, nonfinite_pairs=0, clipped=0, pairs=ints.size // 2)
    np.testing.assert_array_equal(out.cpu().numpy(), ints)
    hist = cf32_histogram(x)
    assert hist.dtype == torch.uint64 and hist.shape == (256,) and hist.is_cuda
    np.testing.assert_array_equal(hist.cpu().numpy(), R.histogram(x))
    assert design_cf32_gain(hist) == 2.0 ** m
    again = cf32_histogram(x[:1000], hist=hist)      # adds into the tensor it is given
    assert again is hist
    np.testing.assert_array_equal(hist.cpu().numpy(), R.histogram(x) + R.histogram(x[:1000]))


def test_a_ci16_capture_over_32768_comes_back_exactly_in_every_form():
    rng = np.random.default_rng(3)
    ints = rng.integers(-32768, 32768, size=2 * 70_001).astype(np.int16)
    ints[:4] = [-32768, 32767, 0, -1]
    x = ints.astype(np.float32) / np.float32(32768.0)
    forms = [x, x.reshape(-1, 2), x.view(np.complex64), x.astype(">f4"), x.view(np.complex64).astype(">c8"), torch.from_numpy(x),
             torch.from_numpy(x).cuda(), torch.from_numpy(x).cuda().view(-1, 2), torch.from_numpy(x.view(np.complex64)).cuda(),
             torch.from_numpy(x).cuda()[2:]]
    for k, form in enumerate(forms):
        out, rep = quantize_cf32(form, full_scale=1.0, return_report=True)
        want = ints[2:] if k == len(forms) - 1 else ints
        assert rep == dict(gain=32768.0, full_scale=1.0, nonfinite_pairs=0, clipped=0, pairs=want.size // 2), k
        np.testing.assert_array_equal(out.cpu().numpy(), want, err_msg=str(k))
    assert torch.equal(quantize_cf32(x, full_scale=1.0), quantize_cf32(x, full_scale=1.0, nonfinite="raise"))
    assert quantize_cf32(x[:0], full_scale=1.0).shape == (0,)
    assert quantize_cf32(x[:0], return_report=True)[1]["gain"] == 1.0
    # float32(32768 / full_scale): UHD's 1.0 is exact, 0.7 is the one rounding of the quotient
    out, rep = quantize_cf32(x, full_scale=0.7, return_report=True)
    assert rep["gain"] == float(np.float32(32768 / 0.7))
    ref_out, ref_bad, ref_clipped = R.quantize(x, np.float32(32768 / 0.7))
    np.testing.assert_array_equal(out.cpu().numpy(), ref_out)
    assert (rep["nonfinite_pairs"], rep["clipped"]) == (ref_bad, ref_clipped) and ref_clipped > 0


def _example():
    spec = importlib.util.spec_from_file_location("classify_capture", os.path.join(ROOT, "examples", "classify_capture.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    return ex


def _same(a, b):
    if isinstance(a, torch.Tensor):
        assert torch.equal(a, b)
    elif isinstance(a, np.ndarray):
        np.testing.assert_array_equal(a, b)
    elif isinstance(a, float) and a != a:
        assert b != b
    else:
        assert a == b


def test_scan_of_the_float_copy_equals_the_scan_of_the_integers(capsys):
    ex = _example()
    ints = ex.synthetic_band("ci16")
    x = ints.astype(np.float32) / np.float32(32768.0)
    back = quantize_cf32(x, full_scale=1.0)
    np.testing.assert_array_equal(back.cpu().numpy(), ints)
    m = VTCNN2.synthetic("deployed3")
    plain, floats = m.scan_iq(torch.from_numpy(ints).cuda(), "ci16", squelch_dbfs=-60.0), m.scan_iq(back, "ci16", squelch_dbfs=-60.0)
    assert len(plain) == len(floats) == 3
    for a, b in zip(plain, floats):
        assert list(a) == list(b)
        for k in a:
            _same(a[k], b[k])
    # 6. the example: --format cf32 --full-scale 1.0 prints the report line and then the integer capture's lines
    capsys.readouterr()
    ex.scan(m, ints, "ci16")
    rows_int = capsys.readouterr().out.strip().splitlines()
    iq, fmt = ex.quantize(x, full_scale=1.0)
    ex.scan(m, iq, fmt)
    rows_float = capsys.readouterr().out.strip().splitlines()
    assert rows_float[0].startswith(f"cf32: {ints.size // 2} pairs, gain 32768 ") and "0 non-finite pairs" in rows_float[0] and "0 components clipped" in rows_float[0]
    assert rows_float[1:] == rows_int and rows_int[0].startswith("3 emitters")
    # measured gain: another power of two, so other integers and another 0 dBFS -- the same emitters, within a bin
    iq, fmt = ex.quantize(x)
    measured = m.scan_iq(iq, fmt, squelch_dbfs=-60.0)
    m._release()
    assert len(measured) == 3
    for a, b in zip(plain, measured):
        assert abs(a["centre"] - b["centre"]) <= 1.0 / 1024


# ---------------------------------------------------------------------------------------------------------------- 5. non-finite input
def test_nonfinite_pairs_are_zeroed_and_counted_or_raise():
    x = (0.1 * np.random.default_rng(9).standard_normal(2 * 5001)).astype(np.float32)
    x[2 * 1234] = np.nan
    out, rep = quantize_cf32(x, full_scale=1.0, return_report=True)
    ref_out, ref_bad, ref_clipped = R.quantize(x, 32768.0)
    np.testing.assert_array_equal(out.cpu().numpy(), ref_out)
    assert (rep["nonfinite_pairs"], rep["clipped"]) == (1, ref_clipped) and out[2 * 1234:2 * 1234 + 2].tolist() == [0, 0]
    for kw in (dict(full_scale=1.0), dict()):
        with pytest.raises(NonFiniteInputError, match="1 component") as info:
            quantize_cf32(x, nonfinite="raise", **kw)
        assert info.value.count == 1
    x[2 * 77 + 1], x[-1] = np.inf, -np.inf
    with pytest.raises(NonFiniteInputError, match="3 component") as info:
        quantize_cf32(torch.from_numpy(x).cuda(), nonfinite="raise")
    assert info.value.count == 3
    # measured gain: the non-finite components are not part of the walk
    out, rep = quantize_cf32(x, return_report=True)
    assert rep["nonfinite_pairs"] == 3 and rep["clipped"] == 0 and rep["gain"] == R.design_gain(R.histogram(x))
    assert 2 ** 13 <= int(out.abs().max()) < 2 ** 14
