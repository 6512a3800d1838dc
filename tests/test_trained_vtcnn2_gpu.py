"""The canonical VT-CNN2 (T3) kernels held to the f64 oracle on a TRAINED net (tests/trained_vtcnn2.py: the DeepSig recipe
from the seed-2016 synthetic weights, on the 11-class frames of tests/signals.py), on held-out frames of a seed training
never saw.  Every other T3 bar was measured on the untrained initialisation, where conv2's sums are random walks, the
softmax is nearly uniform and all frames have alike logits; a trained net has matched conv2 filters (coherent sums: what
the fp8 mode's statistical feature scale assumes away), decisive margins on most frames and thin ones on some.

  * the training gate: the oracle's held-out accuracy at SNR >= 10 dB >= GATE, else every test here fails "net not trained";
  * parity at n = 1, 17, 257, 4,096 in f32, bf16, fp8 and fp8 with bf16 features, at the DEFAULT fp8 input range and
    feature scale (what a user who loads trained weights gets): test_vtcnn2_gpu.TOL against the batch's largest |logit|,
    and TOL_FRAME against each frame's own largest |logit|;
  * the taps (flat, conv, hidden) at test_vtcnn2_gpu.test_taps' bars, and no conv2 feature beyond the E4M3 range;
  * label floors (test_label_agreement_gpu.MODES) against the f32 kernels on 2^16 frames and against the oracle on 4,096;
  * cnn.py's metric, accuracy by SNR, within ACC_BAR of the f32 kernels', whose counts equal the oracle's.
Measured numbers: tools/measure_bars.py --trained -> profiles/r06_measured_bars.json."""
import numpy as np
import pytest
import torch

from modulationdetectioncnn_amd import VTCNN2, Topology
from signals import modulated_frames11
from test_label_agreement_gpu import MODES as FLOORS
from test_vtcnn2_gpu import TOL
import trained_vtcnn2 as T

pytestmark = pytest.mark.gpu

GATE = 0.6
# per-frame bars, |logit err_i| <= TOL_FRAME x max_j |logit_ij|: about twice the largest measured on the 4,096 held-out
# frames (profiles/r06_measured_bars.json: 8.6e-7, 2.6e-3, 4.6e-2, 3.2e-2).  A frame's own largest |logit| is down to 6 %
# of the batch's (p1), so these are the bars that see a frame with small logits go wrong.
TOL_FRAME = {"f32": 2e-6, "bf16": 5e-3, "fp8": 9e-2, "fp8+bf16feat": 6.5e-2}
# per-SNR accuracy (cnn.py's metric) against the f32 kernels' on 2^16 frames (~7,300 per SNR bin): measured 4.1e-4,
# 1.1e-3, 1.2e-3
ACC_BAR = {"bf16": 1e-3, "fp8": 2.5e-3, "fp8+bf16feat": 2.5e-3}
N_FLOOR = 1 << 16
_cache = {}


@pytest.fixture(scope="module")
def net():
    w, st = T.trained()
    assert st["accuracy_snr_ge_10"] >= GATE, f"net not trained: held-out oracle accuracy at SNR >= 10 dB {st['accuracy_snr_ge_10']:.3f} (gate {GATE})"
    return w, st


def _vt(w, mode, **kw):
    m = VTCNN2(Topology.vtcnn2(11), dtype="fp8" if mode.startswith("fp8") else mode, fp8_bf16_features=mode == "fp8+bf16feat", **kw)
    m.set_weights(w)
    return m


def _tol(mode):
    return TOL["fp8" if mode.startswith("fp8") else mode]


def _floor_frames():
    if "floor" not in _cache:
        x, lab, snr = modulated_frames11(N_FLOOR, seed=T.HELD_OUT_SEED + 1)
        _cache["floor"] = (torch.from_numpy(x).cuda(), lab, snr)
    return _cache["floor"]


def _f32_floor(w):
    if "f32" not in _cache:
        x, lab, snr = _floor_frames()
        m = _vt(w, "f32")
        _cache["f32"] = (m.predict_classes(x), m.accuracy_by_snr(x, lab, snr)[0])
    return _cache["f32"]


def test_training_gate(net):
    _, st = net
    print({k: v for k, v in st.items() if k != "classes"})
    assert st["accuracy_snr_ge_10"] >= GATE
    assert st["loss_last_epoch"] < st["loss_first_epoch"]
    assert st["accuracy_by_snr"][18] > st["accuracy_by_snr"][2] or st["accuracy_by_snr"][18] > 0.9


@pytest.mark.parametrize("mode", ["f32", "bf16", "fp8", "fp8+bf16feat"])
@pytest.mark.parametrize("n", [1, 17, 257, 4096])
def test_parity_on_the_trained_net(net, mode, n):
    w, _ = net
    x, _, _, ref = T.held_out()
    x = x[:n]
    rl, rp, rlab = ref["logits"][:n], ref["probs"][:n], ref["labels"][:n]
    m = _vt(w, mode)
    tol, tf = _tol(mode), TOL_FRAME[mode]
    lg = m.predict(x, tap="dense")
    err = np.abs(lg - rl).max(axis=1)
    scale = float(np.abs(rl).max())
    own = np.abs(rl).max(axis=1)
    assert err.max() <= tol * scale, err.max() / scale                       # the batch-relative bar of test_vtcnn2_gpu
    assert (err <= tf * own).all(), float((err / own).max())                 # and each frame against its own logits
    p = m.predict(x)
    assert np.abs(p - rp).max() <= max(2e-6, (2 if mode == "f32" else 0.5) * tol * scale)
    np.testing.assert_allclose(p.sum(axis=1), 1.0, atol=1e-5)
    lab = m.predict_classes(x)
    srt = np.sort(rl, axis=1)
    decided = (srt[:, -1] - srt[:, -2]) > 4 * tf * own
    assert (lab[decided] == rlab[decided]).all(), int((lab[decided] != rlab[decided]).sum())
    assert (lab == np.argmax(p, axis=1)).all()
    if n == 4096 and mode == "f32":
        assert decided.mean() > 0.99, decided.mean()      # (the narrower modes' margins decide fewer frames: all count in the floors)


@pytest.mark.parametrize("mode", ["f32", "bf16", "fp8", "fp8+bf16feat"])
def test_taps_on_the_trained_net(net, mode):
    w, _ = net
    x, _, _, ref = T.held_out()
    x = x[:256]
    m = _vt(w, mode)
    tol = _tol(mode)
    flat = m.predict(x, tap="flat")
    rf = ref["flat"][:256]
    flat_tol = tol + (1.0 / 32 if mode == "fp8" else 0.0)                     # test_vtcnn2_gpu.test_taps' bars
    assert np.abs(flat - rf).max() <= flat_tol * rf.max(), np.abs(flat - rf).max() / rf.max()
    np.testing.assert_array_equal(m.predict(x, tap="conv").reshape(256, -1), flat)
    hid = m.predict(x, tap="hidden")
    assert np.abs(hid - ref["dense1"][:256]).max() <= tol * np.abs(ref["dense1"][:256]).max()


def test_no_fp8_feature_saturates_on_the_trained_net(net):
    """The E4M3 features are the true values x 2^kf, kf = floor(log2(224 / bound)) with the pack's statistical bound; the
    conversion clips at 448 x 2^-kf.  On the trained net's held-out frames no feature of the f64 oracle may lie beyond
    that level, and the fp8 flat tap's largest value must be the oracle's largest, rounded -- not a clipped level below it."""
    w, st = net
    x, _, _, ref = T.held_out()
    kf = int(np.floor(np.log2(224.0 / T.fp8_feature_bound(w))))
    clip = 448.0 * 2.0 ** -kf
    top = float(ref["flat"].max())
    assert top < clip, f"largest feature {top:.4g} beyond the E4M3 range {clip:.4g} (bound {T.fp8_feature_bound(w):.4g})"
    flat = _vt(w, "fp8").predict(x, tap="flat")
    assert flat.max() < clip
    assert abs(float(flat.max()) - top) <= (_tol("fp8") + 1.0 / 16) * top, (float(flat.max()), top)
    # the features the oracle has above half the clip level come out within the rounding of E4M3 + the conv's error
    big = ref["flat"] > 0.5 * clip
    if big.any():
        assert np.abs(flat[big] - ref["flat"][big]).max() <= (_tol("fp8") + 1.0 / 16) * top


@pytest.mark.parametrize("mode,floor", FLOORS)
def test_label_floor_against_the_f32_kernels(net, mode, floor):
    w, _ = net
    x, _, _ = _floor_frames()
    lf, _ = _f32_floor(w)
    agree = float((_vt(w, mode).predict_classes(x) == lf).float().mean())
    assert agree >= floor, f"trained vtcnn2 {mode}: {agree:.5f} of labels equal the f32 kernels' (floor {floor})"


def test_fp8_label_floor_after_calibration(net):
    w, _ = net
    x, _, _ = _floor_frames()
    lf, _ = _f32_floor(w)
    m = _vt(w, "fp8")
    top = m.calibrate_fp8_features(modulated_frames11(256, seed=T.HELD_OUT_SEED + 2)[0])
    assert top > 0.0
    agree = float((m.predict_classes(x) == lf).float().mean())
    assert agree >= 0.985, agree


@pytest.mark.parametrize("mode,floor", FLOORS + [("f32", 0.9995)])
def test_label_floor_against_the_oracle(net, mode, floor):
    w, _ = net
    x, _, _, ref = T.held_out()
    agree = float((_vt(w, mode).predict_classes(x) == ref["labels"]).mean())
    assert agree >= floor, f"trained vtcnn2 {mode}: {agree:.5f} of labels equal the f64 oracle's (floor {floor})"


@pytest.mark.parametrize("mode", ["bf16", "fp8", "fp8+bf16feat"])
def test_accuracy_by_snr_matches_the_f32_kernels(net, mode):
    """cnn.py:228-259's per-SNR accuracy -- the number a user reads -- does not move by more than ACC_BAR in any SNR bin."""
    w, _ = net
    x, lab, snr = _floor_frames()
    _, acc_f = _f32_floor(w)
    acc, conf = _vt(w, mode).accuracy_by_snr(x, lab, snr)
    assert sorted(acc) == sorted(acc_f) == sorted(int(s) for s in np.unique(snr))
    diff = {s: abs(acc[s] - acc_f[s]) for s in acc}
    assert max(diff.values()) <= ACC_BAR[mode], diff
    assert sum(c.sum() for c in conf.values()) == N_FLOOR


def test_f32_accuracy_and_confusion_equal_the_oracles(net):
    """The f32 kernels' accuracy_by_snr and confusion counts are the oracle's labels' exactly, except at numerical ties
    (top-2 margin within 1e-5 of the frame's largest |logit|, where the f32 label may take either class)."""
    w, st = net
    x, lab, snr, ref = T.held_out()
    m = _vt(w, "f32")
    got = m.predict_classes(x)
    srt = np.sort(ref["logits"], axis=1)
    tie = (srt[:, -1] - srt[:, -2]) <= 1e-5 * np.abs(ref["logits"]).max(axis=1)
    assert (got[~tie] == ref["labels"][~tie]).all()
    want = np.where(tie, got, ref["labels"])
    acc, conf = m.accuracy_by_snr(x, lab, snr)
    for s in np.unique(snr):
        sel = snr == s
        c = np.zeros((11, 11), np.int64)
        np.add.at(c, (lab[sel], want[sel]), 1)
        np.testing.assert_array_equal(conf[int(s)], c)
        assert acc[int(s)] == float(np.trace(c)) / sel.sum()
    np.testing.assert_array_equal(m.confusion(x, lab, normalize=False), np.bincount(lab * 11 + want, minlength=121).reshape(11, 11))
    if not tie.any():
        assert acc == pytest.approx(T.accuracy_by_snr(lab, ref["labels"], snr), abs=0)
