"""mdc_iq_synth_capture on the device against the numpy restatement (tests/iq_synth_capture_ref.py), bit for bit and with equal
saturation counts, over every scene of tests/iq_synth_capture_cases.py; then one scene end to end through detect_iq and
score_detections."""
import numpy as np
import pytest

import iq_synth_capture_cases as K
import iq_synth_capture_ref as R
from modulationdetectioncnn_amd import frontend as F

pytestmark = pytest.mark.gpu

_ref = {}


def _want(name, n):
    if (name, n) not in _ref:
        _ref[name, n] = R.scene_capture(K.cases()[name], K.SEED, n)
    return _ref[name, n]


def _run(scene, n, seed=K.SEED):
    out, sat = F.synth_capture(n, scene, seed=seed, return_saturated=True)
    return out.cpu().numpy().reshape(-1, 2), sat


@pytest.mark.parametrize("n", K.LENGTHS)
@pytest.mark.parametrize("name", K.CASE_NAMES)
def test_capture_equals_the_restatement_bit_for_bit(name, n):
    want, want_sat = _want(name, n)
    got, sat = _run(K.cases()[name], n)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"{bad.size} pairs differ, the first at {bad[:8]}: {got[bad[:4]]} != {want[bad[:4]]}"
    assert sat == want_sat
    if name in K.MUST_SATURATE:
        assert sat > 0


@pytest.mark.parametrize("name", ["gauss_and_phase_continuous", "burst_edges", "hopper_8", "E32"])
def test_a_shorter_capture_is_a_prefix(name):
    long, _ = _run(K.cases()[name], 3149)
    short, _ = _run(K.cases()[name], 1500)
    assert np.array_equal(long[:1500], short)
    assert np.array_equal(long, _want(name, 3149)[0])


def test_two_runs_give_the_same_bits_and_another_seed_does_not():
    s = K.cases()["E32"]
    a, b = _run(s, 3072), _run(s, 3072)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    assert not np.array_equal(a[0], _run(s, 3072, seed=K.SEED + 1)[0])


def test_non_default_stream_and_empty_call():
    import torch
    s = K.cases()["gauss_and_phase_continuous"]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        out = F.synth_capture(K.LENGTHS[0], s, seed=K.SEED)
    stream.synchronize()
    assert np.array_equal(out.cpu().numpy().reshape(-1, 2), _want("gauss_and_phase_continuous", K.LENGTHS[0])[0])
    assert F.synth_capture(0, s).numel() == 0


def test_end_to_end_every_whole_dwell_is_found_and_nothing_else():
    """One scene of 2^19 pairs (tests/iq_synth_capture_cases.e2e_scene: a continuous QPSK, a bursty BPSK, a GFSK hopper over four
    carriers, two emitters on the same bins at different times, all 20 dB above the noise inside their bands) through
    synth_capture, VTCNN2.detect_iq(batched=True) with untrained weights and score_detections: every truth dwell that lies wholly
    inside the capture and is at least min_rows = 3 spectrogram rows long is found, and there are no false detections.  The
    numpy references alone meet both conditions on this capture (checked first, on the host: the capture IS the restatement's,
    tests/test_iq_synth_capture.py holds the same on the restatement without a GPU).  Label accuracy is printed, not asserted:
    nothing has been trained."""
    from modulationdetectioncnn_amd import VTCNN2
    scene = K.e2e_scene()
    n = K.E2E_PAIRS
    iq = F.synth_capture(n, scene, seed=K.SEED)
    truth = F.scene_truth(scene, n, K.SEED)
    must = K.e2e_must_find(truth)
    assert len(must) >= 12
    host = F.score_detections(K.numpy_detections(iq.cpu().numpy()), truth)
    assert not set(must) & set(host["missed"]) and host["false"] == []
    model = VTCNN2.synthetic("vtcnn2", classes=len(K.MODS))
    recs = model.detect_iq(iq, "ci16", nfft=K.E2E_NFFT, avg=K.E2E_AVG, batched=True)
    score = F.score_detections(recs, truth, min_overlap=0.5, classes=len(K.MODS))
    print(f"truth dwells {len(truth)}, of them whole and >= 3 rows {len(must)}; detections {len(recs)}; found {len(score['found'])}, "
          f"missed {score['missed']}, false {score['false']}; label accuracy {score['accuracy']:.3f} (untrained weights)")
    model._release()
    assert not set(must) & set(score["missed"])
    assert score["false"] == []
