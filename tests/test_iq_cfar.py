"""mdc_iq_spectrogram_cfar without a GPU: the numpy restatement (tests/iq_cfar_ref.py) against an independent brute-force
statement, the entry point's argument checks (all made before any device call), and the case the feature is for, as conditions
on the restatement -- the kernel inherits them through bit-exactness (tests/test_iq_cfar_gpu.py)."""
import numpy as np
import pytest

import iq_cfar_ref as R
import iq_components_ref as C
from modulationdetectioncnn_amd import _cabi, frontend

MDC_OK, MDC_EINVAL = 0, -22      # include/mdc.h


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("params", [(3, 5, 1, 2, 500), (2, 40, 2, 3, 250), (4, 4, 0, 0, 1000), (0, 3, 0, 1, 0), (16, 2, 3, 2, 999), (5, 9, 1, 9, 700)])
def test_restatement_agrees_with_brute_force(params):
    rng = np.random.default_rng(11)
    P = rng.chisquare(4, (11, 64)).astype(np.float32)
    P[rng.integers(0, 11, 40), rng.integers(0, 64, 40)] = np.float32(1.5)      # ties
    P[3, 7], P[9, 40], P[0, 0] = np.inf, 0.0, np.nan
    P.view(np.uint32)[5, 33] = 0x80000001      # a sign-bit pattern
    f0, q0 = R.cfar(P, *params)
    f1, q1 = R.cfar_brute(P, *params)
    assert np.array_equal(_bits(f0), _bits(f1))
    assert np.array_equal(_bits(q0), _bits(q1))
    assert np.all(np.isin(_bits(f0), np.r_[_bits(P).reshape(-1), np.uint32(0x7F800000)]))      # an element, never an interpolation


def test_restatement_cuts_the_window_off_and_handles_an_empty_training_set():
    P = np.arange(1, 1 + 64, dtype=np.float32).reshape(1, 64)
    P = np.roll(P, -32, axis=1).copy()      # centred column c holds c + 1
    floor, ratio = R.cfar(P, 4, 3, 4, 1, 0)      # one row: the training set is columns c-3, c-2, c+2, c+3 inside the band; the minimum
    fc = np.roll(floor, 32, axis=1)[0]
    assert fc[0] == 3.0 and fc[1] == 4.0 and fc[2] == 1.0 and fc[10] == 8.0 and fc[63] == 61.0      # nothing wraps round
    floor, ratio = R.cfar(P, 4, 2, 0, 2, 500)      # one row, guard as wide as the window: no training cells
    assert np.all(np.isposinf(floor)) and np.all(ratio == 0.0)


def test_frontend_parameter_forms():
    assert frontend.cfar_parameters(None) == (8, 32, 2, 8, 0.5)
    assert frontend.cfar_parameters({"train_bins": 64, "rank": 0.75}) == (8, 64, 2, 8, 0.75)
    assert frontend.cfar_parameters((4, 16, 1, 4, 0.25)) == (4, 16, 1, 4, 0.25)
    with pytest.raises(ValueError):
        frontend.cfar_parameters({"train": 3})
    with pytest.raises(ValueError):
        frontend.cfar_parameters((1, 2, 3))


def test_frontend_refuses_bad_arguments_before_any_device():
    spec = np.zeros((4, 64), np.float32)
    for kw in (dict(train_rows=17), dict(train_bins=129), dict(guard_rows=9), dict(guard_bins=33), dict(guard_rows=-1), dict(guard_bins=-1),
               dict(train_rows=2, train_bins=8), dict(rank=1.5), dict(rank=-0.1), dict(rank=float("nan"))):
        with pytest.raises(ValueError):
            frontend.cfar_floor(spec, **kw)
    with pytest.raises(ValueError):
        frontend.cfar_floor(np.zeros((4, 96), np.float32))
    with pytest.raises(ValueError):
        frontend.cfar_floor(np.zeros((0, 64), np.float32))
    with pytest.raises(TypeError):
        frontend.cfar_floor(np.zeros((4, 64), np.float64))
    with pytest.raises(ValueError):
        frontend.cfar_threshold(100)
    with pytest.raises(ValueError):
        frontend.cfar_threshold(64, threshold_db=float("inf"))


def test_entry_point_validates_its_arguments_without_gpu():
    L = _cabi.lib()
    fn = L.mdc_iq_spectrogram_cfar
    good = dict(rows=16, nfft=256, tr=8, tb=32, gr=2, gb=8, rank=500)

    def call(floor=None, ratio=None, power=None, **kw):
        a = dict(good, **kw)
        return fn(power, a["rows"], a["nfft"], a["tr"], a["tb"], a["gr"], a["gb"], a["rank"], floor, ratio, None)

    assert call() == MDC_OK      # both outputs NULL: nothing is launched
    assert call(tr=16, tb=128, gr=16, gb=127, rank=1000, nfft=4096, rows=(2 ** 31 - 1) // 4096) == MDC_OK      # every limit, reached
    assert call(tr=0, tb=1, gr=0, gb=0, rank=0, nfft=64, rows=1) == MDC_OK
    bad = [dict(rows=0), dict(rows=-3), dict(rows=(2 ** 31 - 1) // 256 + 1), dict(nfft=32), dict(nfft=8192), dict(nfft=96), dict(nfft=0),
           dict(nfft=-64), dict(tr=17), dict(tb=129), dict(gr=9), dict(gb=33), dict(gr=-1), dict(gb=-1), dict(tr=-1, gr=-1), dict(tb=-1, gb=-1),
           dict(tr=2, tb=8), dict(tr=0, tb=0, gr=0, gb=0), dict(rank=-1), dict(rank=1001)]
    for kw in bad:
        assert call(**kw) == MDC_EINVAL, kw
        assert b"mdc_iq_spectrogram_cfar" in L.mdc_last_error()
    # with an output asked for: a NULL input, an output that overlaps the input, a misaligned buffer -- still before any device call
    cells = good["rows"] * good["nfft"]
    assert call(floor=4096) == MDC_EINVAL and call(ratio=4096) == MDC_EINVAL
    assert call(power=4096, floor=4096) == MDC_EINVAL and call(power=4096, ratio=4096 + 4 * (cells - 1)) == MDC_EINVAL
    assert call(power=1 << 20, floor=(1 << 20) - 4 * (cells - 1)) == MDC_EINVAL
    assert call(power=4098, floor=1 << 20) == MDC_EINVAL and call(power=4096, floor=(1 << 20) + 2) == MDC_EINVAL
    assert call(power=4096, floor=1 << 20, ratio=(1 << 21) + 1) == MDC_EINVAL


# ---- the motivating case -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    P, emitter = R.motivating_scene(7)
    return P, emitter


def _score(on_natural, emitter):
    """(share of the noise cells that are on, hit rate per emitter) for a mask in natural positions"""
    on = np.roll(on_natural, on_natural.shape[1] // 2, axis=1)
    noise = emitter < 0
    return float(on[noise].mean()), [float(on[emitter == i].mean()) for i in range(len(R.SCENE_EMITTERS))]


def test_local_floor_keeps_the_noise_off_and_every_emitter_on(scene):
    P, emitter = scene
    assert int((emitter < 0).sum()) == 23744
    _, ratio = R.cfar(P, 8, 32, 2, 8, 500)
    false_share, hits = _score(ratio > R.cfar_threshold(P.shape[1], 6.0, dc_guard=-1)[None, :], emitter)
    print("cfar: false share", false_share, "hit rates", hits)
    assert false_share <= 0.01
    assert min(hits) >= 0.9


@pytest.mark.parametrize("floor", ["flat", "per-bin"])
def test_one_number_per_bin_breaks_a_condition(scene, floor):
    """frontend.detection_threshold's two floors on the same scene: each either switches on more than 1 % of the noise cells or
    misses more than a tenth of some emitter (measured: "flat" 29.7 % false cells, hit rates 0.50 / 1 / 1 / 0.00 -- the burst at the low end is not found;
    "per-bin" 33.6 % false cells, hit rates 0.36 / 0.03 / 1 / 0.06; the local floor: 11 false cells of 23,744, 0.99 / 1 / 1 / 1)."""
    P, emitter = scene
    false_share, hits = _score(P > C.detection_threshold(P, 6.0, dc_guard=-1, floor=floor)[None, :], emitter)
    print(floor, ": false share", false_share, "hit rates", hits)
    assert false_share > 0.01 or min(hits) < 0.9
