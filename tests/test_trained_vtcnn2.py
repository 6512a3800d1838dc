"""The trained-net helper (tests/trained_vtcnn2.py) on the CPU: its training forward, in eval mode, IS the net the f64 oracle
and the kernels compute on the exported weights -- a transposed dense kernel or a channels-last Flatten would make the
"trained" weights look random to them and every trained-net GPU test pass for the wrong reason -- and a few training
steps lower the loss.  The full training runs on the GPU (tests/test_trained_vtcnn2_gpu.py)."""
import numpy as np
import torch

from modulationdetectioncnn_amd import Topology, synthetic_weights
from oracle import oracle_np as O
from signals import modulated_frames11
import trained_vtcnn2 as T


def _perturbed(seed):
    """The seed-2016 start with every tensor moved off its initialisation (non-zero biases, asymmetric kernels), so a
    layout mistake in any layer changes the logits."""
    rng = np.random.default_rng(seed)
    out = []
    for k, b in synthetic_weights(Topology.vtcnn2(11), seed=2016):
        k = k + rng.standard_normal(k.shape).astype(np.float32) * np.abs(k).mean()
        b = (rng.standard_normal(b.shape) * 0.1).astype(np.float32)
        out.append((k, b))
    return out


def test_training_forward_equals_the_oracle_on_the_exported_weights():
    w = _perturbed(3)
    x, _, _ = modulated_frames11(6, seed=4)
    x = x * 20.0      # past the ReLUs' zero region of every layer
    p = T.to_params(w, "cpu")
    with torch.no_grad():
        got = T.forward([t.double() for t in p], torch.from_numpy(x).double(), train=False).numpy()
    ref = O.forward("vtcnn2", x, T.export(p), dtype=np.float64)["logits"]
    scale = np.abs(ref).max()
    assert np.abs(got - ref).max() <= 1e-5 * scale, np.abs(got - ref).max() / scale
    for a, b in zip([t for pair in w for t in pair], [t for pair in T.export(p) for t in pair]):
        np.testing.assert_array_equal(a, b)
    # a deliberately wrong layout is far outside that bar (the check has teeth)
    bad = [(k, b) for k, b in w]
    bad[2] = (w[2][0].reshape(80, 132, 256).transpose(1, 0, 2).reshape(10560, 256), w[2][1])    # channels-last Flatten
    wrong = O.forward("vtcnn2", x, bad, dtype=np.float64)["logits"]
    assert np.abs(wrong - ref).max() > 1e-2 * scale


def test_input_gain_fold_is_exact():
    """Training sees the frames x INPUT_GAIN; the exported net (conv1 x the gain) computes the same on the frames themselves."""
    w = _perturbed(4)
    x, _, _ = modulated_frames11(6, seed=5)
    p = T.to_params(w, "cpu")
    with torch.no_grad():
        got = T.forward([t.double() for t in p], torch.from_numpy(x).double() * T.INPUT_GAIN).numpy()
    folded = T.fold_input_gain(T.export(p))
    np.testing.assert_array_equal(folded[0][0], w[0][0] * np.float32(T.INPUT_GAIN))
    ref = O.forward("vtcnn2", x, folded, dtype=np.float64)["logits"]
    assert np.abs(got - ref).max() <= 1e-9 * np.abs(ref).max()


def test_fp8_bound_restatement_matches_its_definition():
    w = _perturbed(5)
    k1 = w[0][0].astype(np.float64).reshape(256, 3)
    b1, k2, b2 = w[0][1].astype(np.float64), w[1][0].astype(np.float64), w[1][1].astype(np.float64)
    best = 0.0
    for o in range(0, 80, 7):
        var = sum((k2[o, c] ** 2).sum() * (0.02 ** 2 / 16 * (k1[c] ** 2).sum() + b1[c] ** 2) for c in range(256))
        best = max(best, abs(b2[o]) + 12 * np.sqrt(var))
    assert T.fp8_feature_bound(w) >= best * (1 - 1e-12)
    assert T.fp8_feature_bound(w, 0.04) > T.fp8_feature_bound(w)


def test_a_few_training_steps_lower_the_loss():
    w, losses = T.train(n_train=1024, epochs=2, batch=64, device="cpu", steps=24)
    assert len(losses) == 24 and np.isfinite(losses).all()
    assert np.mean(losses[-6:]) < np.mean(losses[:6]) - 0.05, losses
    assert [k.shape for k, _ in w] == [s for s, _ in Topology.vtcnn2(11).layer_shapes]
    assert T.checksum(w) != T.checksum(T.fold_input_gain(synthetic_weights(Topology.vtcnn2(11), seed=2016)))
    assert T.checksum(w) == T.checksum(T.train(n_train=1024, epochs=2, batch=64, device="cpu", steps=24)[0])     # deterministic
