"""Every precision mode against the f64 oracle BIT FOR BIT, on the exact-integer fixtures of tests/exact_fixtures.py.

The parity tests of the matrix-pipe kernels (tests/test_vtcnn2_gpu.py, tests/test_deployed_gpu.py, tests/test_cnnpy_gpu.py)
hold Gaussian data under bars sized to each mode's rounding noise; a fault worth a few 1e-3 of a logit -- one padded edge, one
channel's bias, one k-slice paired with its neighbour's weight, one store a position off -- hides under them.  Here weights and
frames are small integers times a power of two: every sum is exact in f32 in any order, the only roundings left are the narrowing
conversions exact_fixtures.expected() restates (named there with the source lines), and the preconditions are proved on the
oracle before any GPU call.  So taps and labels are compared with ==; the only numeric bar in this file is the project's f32
softmax bar, 2e-6 (tests/test_cnnpy_gpu.py, tests/test_deployed_gpu.py)."""
import numpy as np
import pytest
import torch

import exact_fixtures as X
from modulationdetectioncnn_amd import VTCNN2, Topology

pytestmark = pytest.mark.gpu

SOFTMAX_BAR = 2e-6
_fixtures = {}
_expected = {}


def _fixture(kind, shape, flavour):
    key = (kind, shape, flavour)
    if key not in _fixtures:
        build = {"vtcnn2": lambda: X.vtcnn2_fixture(shape[0], flavour), "deployed": lambda: X.deployed_fixture(shape[0], flavour),
                 "cnnpy": lambda: X.cnnpy_fixture(shape, flavour)}[kind]
        _fixtures[key] = build()
    return _fixtures[key]


def _expect(fx, mode, bf16feat=False):
    """Preconditions first (an AssertionError here is a broken fixture: a test error, never a skip), then the expected arrays."""
    key = (fx.kind, fx.shape, fx.flavour, mode, bf16feat)
    if key not in _expected:
        X.check_preconditions(fx, mode, bf16feat)
        _expected[key] = X.expected(fx, mode, bf16feat)[0]
    return _expected[key]


def _equal(got, want, what):
    got = np.asarray(got)
    want32 = want.astype(np.float32).reshape(got.shape)
    if not np.array_equal(got, want32):
        bad = np.argwhere(got != want32)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.size} elements differ; first at {i}: got {got[i]!r}, oracle {want32[i]!r}")


# ---------------------------------------------------------------------------------------------------------------
# VT-CNN2
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("classes", [11, 16])
@pytest.mark.parametrize("flavour", ["dense", "sparse"])
@pytest.mark.parametrize("mode,bf16feat", X.VT_MODES, ids=["f32", "bf16", "fp8", "fp8-bf16feat"])
def test_vtcnn2_equals_the_oracle_bit_for_bit(mode, bf16feat, flavour, classes):
    """Batches of 1, 17, 257 and 2,304 frames (the last: past the 2,048-frame switch to the head fused into dense1's epilogue,
    and a ragged walk over 256-row GEMM tiles), each a seeded arrangement of the fixture's 64 frames."""
    fx = _fixture("vtcnn2", (classes,), flavour)
    want = _expect(fx, mode, bf16feat)
    kw = dict(fp8_input_absmax=fx.fp8_input_absmax, fp8_bf16_features=bf16feat) if mode == "fp8" else {}
    if mode == "fp8" and not bf16feat:
        kw["fp8_feature_absmax"] = fx.fp8_feature_absmax
    m = VTCNN2(Topology.vtcnn2(classes), dtype=mode, **kw)
    m.set_weights(fx.weights)
    for n in (1, 17, 257, 2304):
        idx = X.batch_indices(n, len(fx.frames), seed=n)
        x = np.ascontiguousarray(fx.frames[idx])
        tag = f"vtcnn2 C={classes} {flavour} {mode}{'+bf16feat' if bf16feat else ''} n={n}"
        flat = m.predict(x, tap="flat")
        _equal(flat, want["flat"][idx], tag + " flat")
        _equal(m.predict(x, tap="conv"), want["conv"][idx], tag + " conv")
        _equal(m.predict(x, tap="hidden"), want["hidden"][idx], tag + " hidden")
        _equal(m.predict(x, tap="dense"), want["dense"][idx], tag + " dense")
        p = m.predict(x)                                          # no tap: above 2,048 frames the fused head, no hidden layer in HBM
        err = float(np.abs(p - want["probs"][idx]).max())
        assert err <= SOFTMAX_BAR, (tag, err)
        lab = m.predict_classes(x)
        assert np.array_equal(lab, want["labels"][idx]), (tag, np.flatnonzero(lab != want["labels"][idx])[:8])
        # the path with taps (dense1 writes the hidden layer, the head is its own launch): same probabilities, same labels
        p_t, l_t, _ = m.forward_device(torch.from_numpy(x).cuda(), tap="dense")
        assert np.array_equal(p_t.cpu().numpy(), p), tag
        assert np.array_equal(l_t.cpu().numpy(), lab), tag


# ---------------------------------------------------------------------------------------------------------------
# deployed nets
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filters", [3, 10])
@pytest.mark.parametrize("flavour", ["dense", "sparse"])
@pytest.mark.parametrize("mode", X.DEP_MODES)
def test_deployed_equals_the_oracle_bit_for_bit(mode, flavour, filters):
    fx = _fixture("deployed", (filters,), flavour)
    want = _expect(fx, mode)
    m = VTCNN2(Topology.deployed(filters), dtype=mode, **(dict(fp8_input_absmax=fx.fp8_input_absmax) if mode == "fp8" else {}))
    m.set_weights(fx.weights)
    for n in (1, 15, 16, 17, 63, 64, 65, 1000):
        idx = X.batch_indices(n, len(fx.frames), seed=n)
        x = np.ascontiguousarray(fx.frames[idx])
        tag = f"deployed F={filters} {flavour} {mode} n={n}"
        if mode == "f32":                                         # the reduced modes reject taps
            _equal(m.predict(x, tap="dense"), want["dense"][idx], tag + " dense")
            _equal(m.predict(x, tap="conv"), want["conv"][idx], tag + " conv")
        err = float(np.abs(m.predict(x) - want["probs"][idx]).max())
        assert err <= SOFTMAX_BAR, (tag, err)
        lab = m.predict_classes(x)
        assert np.array_equal(lab, want["labels"][idx]), (tag, np.flatnonzero(lab != want["labels"][idx])[:8])


# ---------------------------------------------------------------------------------------------------------------
# cnn.py's net on dense_chain
# ---------------------------------------------------------------------------------------------------------------
_CHAIN_BIG = 32768 + 53      # 512 work-groups x 4 waves x 16 rows, then three whole tiles and a ragged one: the smallest batch
                             # at which a wave walks on to a second tile


@pytest.mark.parametrize("flavour", ["dense", "sparse"])
@pytest.mark.parametrize("shape", [(10, 16, 16), (1, 1, 1), (10, 10, 5)])
def test_cnnpy_equals_the_oracle_bit_for_bit(shape, flavour):
    fx = _fixture("cnnpy", shape, flavour)
    x_all = X.cnnpy_frames(_CHAIN_BIG, seed=11)                   # all frames distinct: the oracle is a 256 x 3F product
    X.check_preconditions(fx, frames=x_all)
    want = X.expected(fx, frames=x_all)[0]
    m = VTCNN2(Topology.cnnpy(*shape))
    m.set_weights(fx.weights)
    for n in (1, 16, 17, _CHAIN_BIG):
        x = x_all[:n]
        tag = f"cnnpy {shape} {flavour} n={n}"
        _equal(m.predict(x, tap="conv"), want["conv"][:n], tag + " conv")           # the TAPS instantiation
        _equal(m.predict(x, tap="hidden"), want["hidden"][:n], tag + " hidden")
        _equal(m.predict(x, tap="dense"), want["dense"][:n], tag + " dense")
        err = float(np.abs(m.predict(x) - want["probs"][:n]).max())                 # the no-TAPS instantiation
        assert err <= SOFTMAX_BAR, (tag, err)
        lab = m.predict_classes(x)
        assert np.array_equal(lab, want["labels"][:n]), (tag, np.flatnonzero(lab != want["labels"][:n])[:8])
