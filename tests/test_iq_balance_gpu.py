"""mdc_iq_balance_stats / mdc_iq_balance / frontend.balance / the balance= keyword on the MI355X.  The arithmetic is exact
integers, so every comparison of the two kernels is assert_array_equal against tests/iq_balance_ref.py (numpy int64, written
from include/mdc.h):

  1. statistics: all three formats x B in {64, 65, 255, 256, 1024, 1027, 2^20} x pairs in {0, 1, 3, 4, 5, B-1, B, B+1, 3B+7,
     40,001}; the base pointer one pair into a larger buffer (2-byte alignment for the 8-bit formats, so that heads before the
     first 16-byte boundary occur, and odd B puts blocks on odd pairs); the output pre-filled with a sentinel, one guard row
     after it untouched; inputs uniform over the full range with planted runs of all-minimum, all-maximum and alternating
     pairs; one all-minimum "ci16" block at B = 2^20: sum x^2 = 2^50 exactly;
  2. correction on the same captures: designed coefficients, the identity ("ci16" out == in, 8-bit out == the widening), the
     swap, and the extremes -- dc = +-32768 with rows (32767, 0), (-32767, 0) and (16384, -16383): both clamps are hit --;
     sentinel and guard pair as above; the output at every 4-byte offset from a 16-byte boundary;
  3. one run of each kernel past its grid cap (the stride loops): the whole result against the reference (first, last and all
     between) and against a two-piece run;
  4. two runs are identical, and stats + correction replay bit-identically from a captured graph;
  5. frontend.balance(coeffs=None) == stats -> design on the host -> correction by hand, tensor and numpy input; balance=False
     on predict_iq, scan_iq and detect_iq is bit-identical to not passing it;
  6. the ghost (iq_balance_ref.ghost_scene: a QPSK emitter at +0.18, 41 dB above the floor, a weaker one at -0.33, noise, 1 dB /
     5 degrees and a DC offset; test_iq_balance.py holds the same scene to the same results through the CPU references: the
     image stands 18.4 dB above the floor before, 0.1 dB after, against a threshold of 6 dB): scan_iq lists an emitter inside
     the strong one's bandwidth of -0.18, with balance=True none, the others keep centre (one bin) and label, and
     image_rejection_db is within 0.5 dB of 22.83; detect_iq(balance=True) has no box on the mirrored band;
  7. examples/classify_capture.py's scan on its own imbalanced band prints one row fewer with balance."""
import importlib.util
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import iq_balance_ref as R                                                               # noqa: E402
from conftest import GOLDEN, ROOT                                                        # noqa: E402
from modulationdetectioncnn_amd import VTCNN2, _cabi, frontend                           # noqa: E402

FORMATS = ["cu8", "ci8", "ci16"]
BLOCKS = [64, 65, 255, 256, 1024, 1027, 1 << 20]
SENTINEL = 0x5A5A
SENTINEL64 = 0x5A5A5A5A5A5A5A5A
EXTREMES = [(32768, -32768, 32767, 0, -32767, 0), (-32768, 32768, -32767, 0, 16384, -16383), (32768, 32768, 16384, -16383, 32767, 0),
            (-32768, -32768, 0, 32767, 0, -32767)]


def _pair_counts(B):
    return [0, 1, 3, 4, 5, B - 1, B, B + 1, 3 * B + 7, 40_001]


def _capture(fmt, pairs, seed):
    """One pair of padding + `pairs` pairs + one pair of padding: uniform over the whole range, with runs of 300 pairs of all
    minimum, all maximum and alternating minimum / maximum pairs (cut off where the capture is shorter)"""
    lo, hi, dt = R.SAMPLE_MIN[fmt], R.SAMPLE_MAX[fmt], R.DTYPE[fmt]
    buf = np.random.default_rng(seed).integers(lo, hi + 1, size=2 * (pairs + 2)).astype(dt)
    body = buf[2:-2] if pairs else buf[2:2]
    alt = np.empty(600, dt)
    alt[0::4], alt[1::4], alt[2::4], alt[3::4] = lo, lo, hi, hi
    for at, run in ((0, np.full(600, lo, dt)), (700, np.full(600, hi, dt)), (1500, alt), (max(0, pairs - 200), np.full(600, lo, dt))):
        seg = body[2 * at: 2 * at + 600]
        seg[:] = run[:seg.size]
    return buf


def _on_device(buf):
    """(the whole buffer on the device, the view whose data_ptr is pair 0: one pair in)"""
    whole = torch.from_numpy(buf).cuda()
    return whole, whole[2:]


def _stats(dev, fmt, pairs, B):
    """mdc_iq_balance_stats straight through the binding, with sentinel and guard row; -> (nblocks, 5) numpy"""
    L = _cabi.lib()
    nb = L.mdc_iq_balance_blocks(pairs, B)
    assert nb == R.blocks(pairs, B)
    out = torch.full((nb + 1, 5), SENTINEL64, dtype=torch.int64, device="cuda")
    _cabi.check(L.mdc_iq_balance_stats(dev.data_ptr(), R.FMT[fmt], pairs, B, out.data_ptr(), nb, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert out[nb].tolist() == [SENTINEL64] * 5
    return out[:nb].cpu().numpy()


def _record(c):
    rec = np.zeros((), _cabi.IQ_BALANCE_COEFFS)
    for name, v in zip(_cabi.IQ_BALANCE_COEFFS.names, tuple(c)[:6]):
        rec[name] = int(v)
    return rec


def _correct(dev, fmt, pairs, c):
    """mdc_iq_balance straight through the binding, with sentinel and guard pair; -> (pairs, 2) numpy"""
    out = torch.full((pairs + 1, 2), SENTINEL, dtype=torch.int16, device="cuda")
    rec = _record(c)
    _cabi.check(_cabi.lib().mdc_iq_balance(dev.data_ptr(), R.FMT[fmt], pairs, rec.ctypes.data, out.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert out[pairs].tolist() == [SENTINEL, SENTINEL]
    return out[:pairs].cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------ 1. statistics
@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_stats_bit_for_bit(fmt, B):
    for i, pairs in enumerate(_pair_counts(B)):
        buf = _capture(fmt, pairs, seed=1000 * B % 9973 + i)
        _, dev = _on_device(buf)
        got = _stats(dev, fmt, pairs, B)
        np.testing.assert_array_equal(got, R.stats(buf[2:2 + 2 * pairs], fmt, B), err_msg=f"{fmt} B={B} pairs={pairs}")


def test_stats_of_an_all_minimum_block_reach_2_to_the_50():
    B = 1 << 20
    whole = torch.full((2 * (B + 2),), -32768, dtype=torch.int16, device="cuda")
    got = _stats(whole[2:], "ci16", B, B)
    assert got.tolist() == [[-(1 << 35), -(1 << 35), 1 << 50, 1 << 50, 1 << 50]]


# ------------------------------------------------------------------------------------------------------------------ 2. correction
@pytest.mark.parametrize("fmt", FORMATS)
def test_correction_bit_for_bit(fmt):
    for i, pairs in enumerate(sorted({p for B in (64, 1027) for p in _pair_counts(B)})):
        buf = _capture(fmt, pairs, seed=50 + i)
        _, dev = _on_device(buf)
        body = buf[2:2 + 2 * pairs]
        designed = R.design(R.stats(body, fmt, 1027), pairs)[:6] if pairs else R.IDENTITY
        # a designed matrix of a uniform capture is the identity but for noise: also one of a real imbalance
        for c in [designed, (328, -655, 17462, 720, 720, 15563), R.IDENTITY, R.SWAP, R.CONJUGATE] + EXTREMES:
            got = _correct(dev, fmt, pairs, c)
            np.testing.assert_array_equal(got, R.correct(body, fmt, c), err_msg=f"{fmt} pairs={pairs} c={c}")
        x, y = R.widen(body, fmt)
        np.testing.assert_array_equal(_correct(dev, fmt, pairs, R.IDENTITY), np.stack([x, y], axis=1))
        np.testing.assert_array_equal(_correct(dev, fmt, pairs, R.SWAP), np.stack([y, x], axis=1))


@pytest.mark.parametrize("fmt", FORMATS)
def test_output_aligned_to_one_pair_only(fmt):
    """out_dev wants 4 bytes, no more: whole quads leave as 16 bytes from any such address"""
    pairs, c = 4099, (328, -655, 17462, 720, 720, 15563)
    buf = _capture(fmt, pairs, seed=77)
    _, dev = _on_device(buf)
    rec = _record(c)
    for lead in (1, 2, 3):
        out = torch.full((lead + pairs + 1, 2), SENTINEL, dtype=torch.int16, device="cuda")
        assert out[lead:].data_ptr() % 16 == 4 * lead
        _cabi.check(_cabi.lib().mdc_iq_balance(dev.data_ptr(), R.FMT[fmt], pairs, rec.ctypes.data, out[lead:].data_ptr(),
                                               torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert (got[:lead] == SENTINEL).all() and (got[lead + pairs] == SENTINEL).all()
        np.testing.assert_array_equal(got[lead:lead + pairs], R.correct(buf[2:-2], fmt, c))


def test_extremes_hit_both_clamps():
    buf = _capture("ci16", 40_001, seed=9)
    _, dev = _on_device(buf)
    seen = set()
    for c in EXTREMES:
        got = _correct(dev, "ci16", 40_001, c)
        seen |= {int(got.min()), int(got.max())}
        x, y = R.widen(buf[2:-2], "ci16")
        pre = c[2] * (x - c[0]) + c[3] * (y - c[1]) + 8192
        assert (pre >> 14).max() > 32767 or (pre >> 14).min() < -32768      # the clamp worked, not the range
    assert {-32768, 32767} <= seen


# ---------------------------------------------------------------------------------------------------------------- 3. stride loops
def test_stats_stride_loop():
    B = 64
    nblocks = 2 * _cabi.BALANCE_STATS_GRID_CAP + 37
    pairs = (nblocks - 1) * B + 5
    buf = _capture("ci8", pairs, seed=21)
    _, dev = _on_device(buf)
    got = _stats(dev, "ci8", pairs, B)
    assert got.shape[0] == nblocks > _cabi.BALANCE_STATS_GRID_CAP
    np.testing.assert_array_equal(got, R.stats(buf[2:-2], "ci8", B))
    cut = 1001 * B      # two pieces, split on the block grid
    np.testing.assert_array_equal(got, np.concatenate([_stats(dev, "ci8", cut, B), _stats(dev[2 * cut:], "ci8", pairs - cut, B)]))


def test_correction_stride_loop():
    pairs = 2 * _cabi.BALANCE_GRID_CAP * _cabi.BALANCE_GROUP_PAIRS + 4099
    buf = _capture("cu8", pairs, seed=22)
    _, dev = _on_device(buf)
    c = (-300, 411, 17462, 720, 720, 15563)
    got = _correct(dev, "cu8", pairs, c)
    np.testing.assert_array_equal(got, R.correct(buf[2:-2], "cu8", c))
    cut = 1_234_567      # two pieces, split off every grid
    np.testing.assert_array_equal(got, np.concatenate([_correct(dev, "cu8", cut, c), _correct(dev[2 * cut:], "cu8", pairs - cut, c)]))


# ------------------------------------------------------------------------------------------------- 4. determinism and graph replay
def test_runs_are_identical_and_replay_from_a_graph():
    fmt, pairs, B = "ci16", 200_003, 1027
    c = (328, -655, 17462, 720, 720, 15563)
    L, rec = _cabi.lib(), _record(c)
    nb = L.mdc_iq_balance_blocks(pairs, B)
    whole, dev = _on_device(_capture(fmt, pairs, seed=31))
    first = (_stats(dev, fmt, pairs, B), _correct(dev, fmt, pairs, c))
    again = (_stats(dev, fmt, pairs, B), _correct(dev, fmt, pairs, c))
    np.testing.assert_array_equal(first[0], again[0])
    np.testing.assert_array_equal(first[1], again[1])
    sums = torch.empty((nb, 5), dtype=torch.int64, device="cuda")
    out = torch.empty((pairs, 2), dtype=torch.int16, device="cuda")
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        s = torch.cuda.current_stream().cuda_stream
        _cabi.check(L.mdc_iq_balance_stats(dev.data_ptr(), R.FMT[fmt], pairs, B, sums.data_ptr(), nb, s))
        _cabi.check(L.mdc_iq_balance(dev.data_ptr(), R.FMT[fmt], pairs, rec.ctypes.data, out.data_ptr(), s))
    for seed in (32, 33):
        buf = _capture(fmt, pairs, seed=seed)
        whole.copy_(torch.from_numpy(buf).cuda())      # same buffer, new capture
        sums.fill_(-1)
        out.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(sums.cpu().numpy(), R.stats(buf[2:-2], fmt, B))
        np.testing.assert_array_equal(out.cpu().numpy(), R.correct(buf[2:-2], fmt, c))


# ------------------------------------------------------------------------------------------------------------- 5. the Python layer
def _net():
    return VTCNN2.from_npz(os.path.join(GOLDEN, "weights", "3convmodrecnets_CNN2_0.5.npz"))


@pytest.mark.parametrize("fmt", FORMATS)
def test_frontend_balance_is_stats_design_correction(fmt):
    pairs = 70_001
    rng = np.random.default_rng(41)
    z = 0.3 * np.exp(2j * np.pi * 0.1837 * np.arange(pairs)) + 0.01 * (rng.standard_normal(pairs) + 1j * rng.standard_normal(pairs))
    iq = R.quantise(R.impair(z, 1.0, 5.0, 0.02 - 0.01j), fmt)
    sums = frontend.balance_stats(iq, fmt, block_pairs=4099)
    assert sums.shape == (18, 5) and sums.dtype == torch.int64 and sums.is_cuda and sums.pairs == pairs
    np.testing.assert_array_equal(sums.cpu().numpy(), R.stats(iq, fmt, 4099))
    c = frontend.design_balance(sums)
    assert tuple(c) == R.design(R.stats(iq, fmt, 4099), pairs)
    assert frontend.image_rejection_db(sums) == pytest.approx(R.image_rejection_db(R.stats(iq, fmt, 4099), pairs), abs=1e-9)
    by_hand = R.correct(iq, fmt, c)
    for src in (iq, torch.from_numpy(iq).cuda(), iq.reshape(-1, 2)):
        got = frontend.balance(src, fmt, block_pairs=4099)
        assert got.shape == (pairs, 2) and got.dtype == torch.int16 and got.is_cuda
        np.testing.assert_array_equal(got.cpu().numpy(), by_hand)
        np.testing.assert_array_equal(frontend.balance(src, fmt, coeffs=c).cpu().numpy(), by_hand)
        np.testing.assert_array_equal(frontend.balance(src, fmt, coeffs=tuple(c)[:6]).cpu().numpy(), by_hand)
    out, used, irr = frontend.balance(iq, fmt, return_coeffs=True)
    assert used == frontend.design_balance(R.stats(iq, fmt, 65536), pairs) and abs(irr - 22.83) < 0.1
    assert frontend.balance(iq, fmt, coeffs=c, return_coeffs=True)[2] is None
    assert frontend.balance(iq[:0], fmt).shape == (0, 2)
    np.testing.assert_array_equal(frontend.balance(iq, fmt, coeffs=frontend.BALANCE_SWAP).cpu().numpy(), R.correct(iq, fmt, R.SWAP))


def _same(a, b):
    if isinstance(a, torch.Tensor):
        assert torch.equal(a, b)
    elif isinstance(a, np.ndarray):
        np.testing.assert_array_equal(a, b)
    elif isinstance(a, float) and a != a:
        assert b != b
    else:
        assert a == b


@pytest.fixture(scope="module")
def ghost():
    """(the net, the scene on the device, scan_iq's records without the keyword)"""
    m = _net()
    dev = torch.from_numpy(R.ghost_scene()).cuda()
    yield m, dev, m.scan_iq(dev, "ci16", squelch_dbfs=-60.0)
    m._release()


def test_balance_false_changes_nothing(ghost):
    m, dev, plain = ghost
    off = m.scan_iq(dev, "ci16", squelch_dbfs=-60.0, balance=False)
    assert len(off) == len(plain)
    for a, b in zip(plain, off):
        assert list(a) == list(b) and "image_rejection_db" not in a
        for k in a:
            _same(a[k], b[k])
    part = dev[:2 * 65536]
    for a, b in zip(m.detect_iq(part, "ci16"), m.detect_iq(part, "ci16", balance=False)):
        assert list(a) == list(b) and "image_rejection_db" not in a
        for k in a:
            _same(a[k], b[k])
    kw = dict(normalize="rms", return_power=True)
    for src in (part, part.cpu().numpy()):
        for a, b in zip(m.predict_iq(src, "ci16", **kw), m.predict_iq(src, "ci16", balance=False, **kw)):
            _same(a, b)
    # and True is the correction in front of the same call
    fixed = frontend.balance(part, "ci16").view(-1)
    for a, b in zip(m.predict_iq(fixed, "ci16", **kw), m.predict_iq(part, "ci16", balance=True, **kw)):
        _same(a, b)
    for a, b in zip(m.predict_iq(fixed, "ci16", **kw), m.predict_iq(part.cpu().numpy(), "ci16", balance=True, **kw)):
        np.testing.assert_array_equal(a.cpu().numpy(), b)
    M = 16
    for a, b in zip(m.predict_channels(fixed, "ci16", M), m.predict_channels(part, "ci16", M, balance=True)):
        _same(a, b)


# --------------------------------------------------------------------------------------------------------------------- 6. the ghost
def test_the_ghost_is_listed_without_balance_and_gone_with_it(ghost):
    m, dev, plain = ghost
    sps, fc, _ = R.GHOST_STRONG
    bw = 1.35 / sps
    ghosts = [e for e in plain if abs(e["centre"] + fc) <= bw]
    assert len(ghosts) == 1, [e["centre"] for e in plain]
    fixed = m.scan_iq(dev, "ci16", squelch_dbfs=-60.0, balance=True)
    assert not [e for e in fixed if abs(e["centre"] + fc) <= bw], [e["centre"] for e in fixed]
    others = [e for e in plain if abs(e["centre"] + fc) > bw]
    assert len(fixed) == len(others) == 2
    for a, b in zip(others, fixed):
        assert abs(a["centre"] - b["centre"]) <= 1.0 / 1024 and a["label"] == b["label"]
        assert abs(b["image_rejection_db"] - 22.83) <= 0.5
    given = m.scan_iq(dev, "ci16", squelch_dbfs=-60.0, balance=frontend.balance(dev, "ci16", return_coeffs=True)[1])
    assert [e["centre"] for e in given] == [e["centre"] for e in fixed] and all(e["image_rejection_db"] is None for e in given)


def test_detect_iq_has_no_box_on_the_mirrored_band(ghost):
    m, dev, _ = ghost
    sps, fc, _ = R.GHOST_STRONG
    lo, hi = -fc - 1.35 / sps / 2, -fc + 1.35 / sps / 2

    def on_mirror(records):
        return [d for d in records if d["centre"] - d["bandwidth"] / 2 < hi and d["centre"] + d["bandwidth"] / 2 > lo]
    assert on_mirror(m.detect_iq(dev, "ci16", batched=True))      # the scene does need the correction
    fixed = m.detect_iq(dev, "ci16", batched=True, balance=True)
    assert fixed and not on_mirror(fixed)
    assert all(abs(d["image_rejection_db"] - 22.83) <= 0.5 for d in fixed)


# ------------------------------------------------------------------------------------------------------------------- 7. the example
def test_example_scan_prints_one_row_fewer_with_balance(capsys):
    spec = importlib.util.spec_from_file_location("classify_capture", os.path.join(ROOT, "examples", "classify_capture.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    iq = ex.synthetic_band("ci16", emitters=ex.IMBALANCED_EMITTERS, imbalance=ex.IMBALANCE)
    m = VTCNN2.synthetic("deployed3")
    ex.scan(m, iq, "ci16")
    rows_plain = capsys.readouterr().out.strip().splitlines()
    ex.scan(m, iq, "ci16", balance=True)
    rows_balanced = capsys.readouterr().out.strip().splitlines()
    m._release()
    assert rows_plain[0].startswith("4 emitters") and rows_balanced[0].startswith("3 emitters") and "image rejection" in rows_balanced[0]
    assert len(rows_balanced) == len(rows_plain) - 1
