"""mdc_iq_spectrogram_cfar / frontend.cfar_floor / VTCNN2.detect_iq(floor="cfar") on the MI355X: floor and ratio bit for bit against
the numpy restatement (tests/iq_cfar_ref.py) at every shape, parameter set and kind of value the kernel can go wrong on; the
outputs one at a time; through the component kernel; and end to end on a capture with a gain step.

Shapes: the kernel's tile is 16 rows x 64 centred columns, a lane owns 4 consecutive rows of a column.  rows = 1 and 5 (less than
train_rows, less than a tile), 19 x 64 (one column tile, a row-tile seam, a tail of 3 rows: not a multiple of 4; train_bins = 40
is wider than half the band), 37 x 128 (row and column tile seams), 9 x 4096 (the widest row), 40 x 512 at train (16, 128) (the
LDS maximum, 60 KB)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import iq_cfar_cases as K            # noqa: E402
import iq_cfar_ref as R              # noqa: E402
import iq_components_ref as C        # noqa: E402
import signals                       # noqa: E402
from modulationdetectioncnn_amd import _cabi, frontend as F      # noqa: E402

DEFAULT = (8, 32, 2, 8, 500)


def _i32(t):
    return (t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))).view(torch.int32).cpu()


def _gpu(P, params, ratio=True):
    tr, tb, gr, gb, permille = params
    return F.cfar_floor(torch.from_numpy(P).cuda(), tr, tb, gr, gb, rank=permille / 1000.0, return_ratio=ratio)


def _hold(P, params):
    """floor and ratio of the device against the restatement, bit for bit; returns the restatement's"""
    want_floor, want_ratio = R.cfar(P, *params)
    floor, ratio = _gpu(P, params)
    torch.cuda.synchronize()
    assert floor.shape == ratio.shape == P.shape and floor.dtype == ratio.dtype == torch.float32
    bad = (_i32(floor) != _i32(want_floor)).nonzero()
    assert bad.numel() == 0, (params, P.shape, "floor differs first at", bad[0].tolist(), "in", int(bad.shape[0]), "cells")
    bad = (_i32(ratio) != _i32(want_ratio)).nonzero()
    assert bad.numel() == 0, (params, P.shape, "ratio differs first at", bad[0].tolist(), "in", int(bad.shape[0]), "cells")
    assert torch.equal(_i32(floor), _i32(want_floor)) and torch.equal(_i32(ratio), _i32(want_ratio))
    return want_floor, want_ratio


def _noise(shape, seed):
    """a spectrogram's values: chi-square, 16 degrees of freedom, on a 20 dB slope"""
    rng = np.random.default_rng(seed)
    return (rng.chisquare(16, shape) / 16.0 * 10.0 ** (2.0 * np.arange(shape[1]) / shape[1])).astype(np.float32)


# ---- shapes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,params", [((1, 64), DEFAULT), ((1, 256), DEFAULT), ((5, 128), DEFAULT), ((19, 64), (8, 40, 2, 8, 500)),
                                          ((37, 128), DEFAULT), ((9, 4096), DEFAULT), ((16, 64), DEFAULT), ((33, 256), (3, 70, 1, 2, 250))])
def test_shapes(shape, params):
    _hold(_noise(shape, 3), params)


# ---- parameters ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,params", [((21, 128), (4, 20, 4, 5, 500)),      # guard_rows == train_rows, guard_bins < train_bins
                                          ((21, 128), (6, 9, 2, 9, 500)),       # the reverse
                                          ((21, 128), (5, 12, 0, 0, 500)),      # guard (0, 0): the cell alone
                                          ((40, 512), (16, 128, 2, 8, 500)),    # the LDS maximum
                                          ((40, 512), (16, 128, 16, 127, 900)),
                                          ((7, 64), (0, 3, 0, 1, 500)),         # one row only
                                          ((7, 64), (0, 3, 0, 0, 1000)),
                                          ((3, 64), (16, 128, 0, 0, 500)),      # the window holds the whole spectrogram
                                          ((23, 128), (8, 32, 2, 8, 0)), ((23, 128), (8, 32, 2, 8, 999)), ((23, 128), (8, 32, 2, 8, 1000)),
                                          ((23, 128), (8, 32, 2, 8, 1)), ((23, 128), (2, 1, 1, 0, 333))])
def test_parameters(shape, params):
    _hold(_noise(shape, 5), params)


def test_an_empty_training_set_is_plus_infinity():
    P = _noise((1, 64), 9)
    floor, ratio = _hold(P, (4, 2, 0, 2, 500))      # one row, the guard as wide as the window
    assert np.all(np.isposinf(floor)) and np.all(ratio == 0.0)


# ---- values -------------------------------------------------------------------------------------------------------------------------
def test_random_bit_patterns_nan_and_sign_bit_included():
    rng = np.random.default_rng(17)
    P = rng.integers(0, 1 << 32, (25, 128), dtype=np.uint64).astype(np.uint32).view(np.float32)
    assert np.isnan(P).any() and (P.view(np.uint32) >> 31).any() and (np.abs(P[np.isfinite(P)]) < 1.2e-38).any()
    for params in (DEFAULT, (3, 5, 1, 1, 0), (3, 5, 1, 1, 1000)):
        _hold(P, params)


def test_all_zero():
    P = np.zeros((18, 64), np.float32)
    floor, ratio = _hold(P, DEFAULT)
    assert np.all(floor.view(np.uint32) == 0) and np.all(np.isnan(ratio))


def test_three_values_only_ties_everywhere():
    rng = np.random.default_rng(23)
    P = rng.choice(np.array([0.5, 1.0, 4.0], np.float32), (29, 128))
    for permille in (0, 333, 500, 667, 1000):
        _hold(P, (8, 32, 2, 8, permille))


def test_a_column_of_infinity():
    P = _noise((20, 128), 29)
    P[:, 37] = np.inf
    P[4, 90], P[11, 91] = np.inf, 0.0
    floor, ratio = _hold(P, (2, 1, 0, 0, 1000))      # the maximum of eight or fewer neighbours: the column is the floor next to it
    assert np.isinf(floor).any() and np.isnan(ratio).any() and (ratio == 0.0).any()
    _hold(P, DEFAULT)


def test_the_real_thing_a_spectrogram_of_modulated_frames():
    frames, _, _ = signals.modulated_frames(128, seed=7)
    z = np.stack([frames[:, 0, :].reshape(-1), frames[:, 1, :].reshape(-1)], axis=1).reshape(-1).astype(np.float64)
    iq = np.rint(z / np.abs(z).max() * 12000).astype(np.int16)
    spec = F.spectrogram(torch.from_numpy(iq).cuda(), "ci16", nfft=64, avg=2)
    P = spec.cpu().numpy()
    assert P.shape[0] > 100 and P.shape[1] == 64
    want_floor, want_ratio = R.cfar(P, 8, 20, 2, 4, 500)
    floor, ratio = F.cfar_floor(spec, 8, 20, 2, 4, 0.5, return_ratio=True)      # the device tensor as it comes
    assert torch.equal(_i32(floor), _i32(want_floor)) and torch.equal(_i32(ratio), _i32(want_ratio))


def test_the_band_is_not_circular():
    P = np.ones((12, 128), np.float32)
    P[:, (0 + 64) % 128] = 1000.0      # centred column 0 is natural bin nfft/2
    floor, _ = _hold(P, (2, 3, 0, 0, 1000))      # the maximum of the neighbours: the spike shows in every floor that sees it
    fc = np.roll(floor, 64, axis=1)
    assert np.all(fc[:, 1:4] == 1000.0) and np.all(fc[:, 4:] == 1.0)
    assert np.all(fc[:, 127] == 1.0)      # centred column nfft - 1 is the other END of the band, not a neighbour


# ---- outputs ------------------------------------------------------------------------------------------------------------------------
def test_one_output_at_a_time_and_twice_the_same_bits():
    P = _noise((37, 128), 31)
    dev = torch.from_numpy(P).cuda()
    floor, ratio = _gpu(P, DEFAULT)
    again = _gpu(P, DEFAULT)
    assert torch.equal(_i32(floor), _i32(again[0])) and torch.equal(_i32(ratio), _i32(again[1]))
    assert torch.equal(_i32(F.cfar_floor(dev)), _i32(floor))      # ratio_dev NULL
    lib, stream = _cabi.lib(), torch.cuda.current_stream().cuda_stream
    only = torch.full_like(ratio, -7.0)
    _cabi.check(lib.mdc_iq_spectrogram_cfar(dev.data_ptr(), 37, 128, 8, 32, 2, 8, 500, None, only.data_ptr(), stream))      # floor_dev NULL
    torch.cuda.synchronize()
    assert torch.equal(_i32(only), _i32(ratio))
    assert lib.mdc_iq_spectrogram_cfar(dev.data_ptr(), 37, 128, 8, 32, 2, 8, 500, None, None, stream) == 0
    assert torch.equal(dev.cpu(), torch.from_numpy(P))      # the input is only read


def test_the_call_is_capturable_and_replays_bit_identically():
    """tests/test_graph_capture_gpu.py's pattern: warm on a side stream, capture the call there, replay on new contents of the same
    buffers"""
    rows, nfft = 37, 256
    dev = torch.from_numpy(_noise((rows, nfft), 41)).cuda()
    floor, ratio = torch.empty_like(dev), torch.empty_like(dev)
    lib = _cabi.lib()

    def enqueue():
        _cabi.check(lib.mdc_iq_spectrogram_cfar(dev.data_ptr(), rows, nfft, 8, 32, 2, 8, 500, floor.data_ptr(), ratio.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        enqueue()
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        enqueue()
    for seed in (42, 43):
        P = _noise((rows, nfft), seed)
        dev.copy_(torch.from_numpy(P))
        floor.zero_()
        ratio.zero_()
        g.replay()
        torch.cuda.synchronize()
        want_floor, want_ratio = R.cfar(P, *DEFAULT)
        assert torch.equal(_i32(floor), _i32(want_floor)) and torch.equal(_i32(ratio), _i32(want_ratio)), seed


# ---- through the components ---------------------------------------------------------------------------------------------------------
def test_find_detections_on_the_ratio_equals_the_references():
    P, _ = R.motivating_scene(7)
    _, want_ratio = R.cfar(P, *DEFAULT)
    thresh = R.cfar_threshold(P.shape[1], 6.0, 1)
    _, records, count = C.components(want_ratio, thresh, 2, 3)
    want = C.find_detections(want_ratio, thresh, records, count, avg=8)
    assert len(want) >= 4
    ratio = F.cfar_floor(torch.from_numpy(P).cuda(), return_ratio=True)[1]
    dev_thresh = F.cfar_threshold(P.shape[1], 6.0, 1)
    assert torch.equal(_i32(dev_thresh), _i32(thresh))
    got = F.find_detections(ratio, dev_thresh, avg=8)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert tuple(g[:5]) == tuple(w[:5]) and tuple(g[9:]) == tuple(w[9:])      # the box, the cells, the pairs: exact
        np.testing.assert_allclose(np.array(g[5:9]), np.array(w[5:9]), rtol=1e-12, atol=1e-12)      # float64 sums of the same numbers


# ---- end to end: a gain step ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stepped():
    quiet, loud = K.scenes()
    iq = torch.cat([F.synth_capture(K.HALF_PAIRS, quiet, seed=K.SEED), F.synth_capture(K.HALF_PAIRS, loud, seed=K.SEED)])
    return iq, K.truth()


def _mostly_loud(rec):
    return max(rec["stop_pair"] - max(rec["first_pair"], K.HALF_PAIRS), 0) > (rec["stop_pair"] - rec["first_pair"]) / 2


def test_end_to_end_across_a_gain_step(stepped):
    """Two renders of one scene, the second 10 dB up (2^18 pairs in all).  detect_iq(floor="cfar"): batched and loop agree key
    for key; every truth burst that is whole, at least 3 rows long and at least train_rows rows from the seam is found; the
    false detections are those of the same chain on the restatement's floor (the same list).  floor="flat" on the same capture
    leaves a false detection in the loud half: the case the feature is for."""
    from modulationdetectioncnn_amd import VTCNN2
    iq, truth = stepped
    must = K.must_find(truth)
    assert len(must) >= 12 and any(truth["first_pair"][t] >= K.HALF_PAIRS for t in must) and any(truth["stop_pair"][t] <= K.HALF_PAIRS for t in must)
    model = VTCNN2.synthetic("vtcnn2", classes=len(K.MODS))
    recs = model.detect_iq(iq, "ci16", nfft=K.NFFT, avg=K.AVG, floor="cfar", batched=True)
    loop = model.detect_iq(iq, "ci16", nfft=K.NFFT, avg=K.AVG, floor="cfar")
    named = model.detect_iq(iq, "ci16", nfft=K.NFFT, avg=K.AVG, floor="cfar", cfar=dict(train_rows=8, train_bins=32, guard_rows=2, guard_bins=8, rank=0.5),
                            batched=True)
    with pytest.raises(ValueError):
        model.detect_iq(iq, "ci16", nfft=K.NFFT, avg=K.AVG, floor="flat", cfar=(8, 32, 2, 8, 0.5))
    with pytest.raises(ValueError):
        model.detect_iq(iq, "ci16", nfft=K.NFFT, avg=K.AVG, floor="local")
    model._release()
    assert len(recs) == len(loop) == len(named)
    for a, b, c in zip(recs, loop, named):
        assert list(a) == list(b) == list(c)
        for key in a:
            for other in (b, c):
                if isinstance(a[key], torch.Tensor):
                    assert torch.equal(a[key], other[key]), key
                else:
                    assert a[key] == other[key], key
    score = F.score_detections(recs, truth)
    # the same chain on the restatement's floor
    spec = F.spectrogram(iq, "ci16", nfft=K.NFFT, avg=K.AVG)
    # floor="flat": detect_iq's own search lines (its boxes across the whole loud half are too wide for a channel plan, so the
    # search is taken without the classifier behind it)
    flat = [d._asdict() for d in F.find_detections(spec, F.detection_threshold(spec, 6.0, 1, "flat"), 2, 3, 3, 3, avg=K.AVG)]
    P = spec.cpu().numpy()
    _, want_ratio = R.cfar(P, *DEFAULT)
    thresh = R.cfar_threshold(K.NFFT, 6.0, 1)
    _, records, count = C.components(want_ratio, thresh, 2, 3)
    host = [d._asdict() for d in F.detections_from_components(want_ratio, thresh, records.view(_cabi.IQ_COMPONENT), count, avg=K.AVG)]
    host_score = F.score_detections(host, truth)
    flat_score = F.score_detections(flat, truth)
    flat_false = [i for i in flat_score["false"] if _mostly_loud(flat[i])]
    print(f"truth {len(truth)}, must {len(must)}; cfar: detections {len(recs)}, missed {score['missed']}, false {score['false']}; on the restatement's "
          f"floor: detections {len(host)}, false {host_score['false']}; flat: detections {len(flat)}, missed {flat_score['missed']}, false {flat_score['false']}")
    assert not set(must) & set(score["missed"])
    assert [tuple(r[k] for k in ("first_row", "stop_row", "first_bin", "stop_bin", "cells")) for r in recs] == \
           [tuple(r[k] for k in ("first_row", "stop_row", "first_bin", "stop_bin", "cells")) for r in host]
    assert score["false"] == host_score["false"]
    assert len(flat_false) >= 1
