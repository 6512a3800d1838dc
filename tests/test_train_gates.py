"""The gates fixtures of tests/train_gates.py, on the CPU: every fixture meets its preconditions on the f64 oracle; every
mutant -- the oracle with ONE named fault, the faults a training kernel could have at its decision points -- leaves the true
oracle on some fixture by at least 100x the bar tests/test_train_gates_gpu.py applies to that tensor; and the oracle itself
agrees with torch autograd on these batches (soft rows and clipped frames inside the full nets, not only in
crossentropy_on_probs)."""
import numpy as np
import pytest
import torch

from oracle import oracle_train as T
from tests import train_gates as G
from tests.test_oracle_train import _torch_loss

SEEN = 100.0      # a mutant counts as seen where it differs by this many bars


@pytest.mark.parametrize("kind,shape", G.TOPOLOGIES, ids=G.TOPOLOGY_IDS)
def test_every_fixture_meets_its_preconditions(kind, shape):
    for n in G.MIXED_COUNTS:
        counts = G.check_preconditions(G.mixed(kind, shape, n))
        assert min(counts.values()) >= G.MIN_PER_CATEGORY
    for category in G.PURE_KINDS:
        if category == "dead" and kind != "deployed":
            continue
        for n in G.PURE_COUNTS:
            assert G.check_preconditions(G.pure(kind, shape, category, n))[category] == n


@pytest.mark.parametrize("kind,shape", G.TOPOLOGIES, ids=G.TOPOLOGY_IDS)
def test_the_shuffled_batch_is_the_batch_and_a_dropout_seed_exists(kind, shape):
    for n in G.MIXED_COUNTS:
        fx = G.mixed(kind, shape, n)
        xr, yr, order, first = G.shuffled(fx)
        assert first != 0 and len(order) == first + n
        assert np.array_equal(xr[order[first:]], fx.frames) and np.array_equal(yr[order[first:]], fx.targets)
        assert not np.array_equal(order[first:], np.arange(n))
        assert 1 <= G.dropout_seed(fx) <= 64


def test_a_broken_fixture_is_an_error():
    """check_preconditions does look: a frame moved into a grey zone, a gate moved next to zero, a conv bias, a missing category."""
    fx = G.mixed("deployed", (3,), 17)
    grey = G.Gates(fx.kind, fx.shape, "grey", [fx.weights[0], (fx.weights[1][0], np.array([14.0, 0.0, -0.4], np.float32))], fx.frames, fx.targets)
    with pytest.raises(AssertionError, match="grey zone"):      # silent frames: q = softmax(14, 0, 0) -> 8e-7
        G.check_preconditions(grey)
    near = G.Gates(fx.kind, fx.shape, "near", [fx.weights[0], (fx.weights[1][0], np.array([0.7, 1e-3, -0.4], np.float32))], fx.frames, fx.targets)
    with pytest.raises(AssertionError, match="'z' pre-activation"):
        G.check_preconditions(near)
    biased = G.Gates(fx.kind, fx.shape, "biased", [(fx.weights[0][0], np.full(3, 0.25, np.float32)), fx.weights[1]], fx.frames, fx.targets)
    with pytest.raises(AssertionError, match="conv bias"):
        G.check_preconditions(biased)
    hot = fx.targets.copy()
    hot[~G._is_onehot(hot.astype(np.float64))] = [1, 0, 0]
    with pytest.raises(AssertionError, match="'soft' frames"):
        G.check_preconditions(G.Gates(fx.kind, fx.shape, "no-soft", fx.weights, fx.frames, hot))
    with pytest.raises(AssertionError, match="not every frame"):
        G.check_preconditions(G.Gates(fx.kind, fx.shape, "not-pure", fx.weights, fx.frames, fx.targets, pure="low"))


@pytest.mark.parametrize("kind,shape", [G.TOPOLOGIES[0], G.TOPOLOGIES[2]], ids=[G.TOPOLOGY_IDS[0], G.TOPOLOGY_IDS[2]])
def test_the_mutants_without_a_fault_are_the_oracle(kind, shape):
    fx = G.mixed(kind, shape, 93)
    loss, grads = G.mutant_loss_and_grads(kind, fx.frames, fx.targets, fx.weights, None)
    ref_loss, _li, ref, _p = T.loss_and_grads(kind, fx.frames, fx.targets, fx.weights, np.float64)
    assert loss == ref_loss
    for (gk, gb), (rk, rb) in zip(grads, ref):
        assert np.array_equal(gk, rk) and np.array_equal(gb, rb)


def _fixtures_of(kind):
    for k, shape in G.TOPOLOGIES:
        if k == kind:
            for n in G.MIXED_COUNTS:
                yield G.mixed(k, shape, n)


@pytest.mark.parametrize("kind,fault", [(k, f) for k in ("deployed", "cnnpy") for f in G.GRAD_FAULTS[k]])
def test_every_gradient_mutant_is_seen_at_100_bars(kind, fault):
    """For each fault there is a mixed fixture and a tensor (or the loss) where the faulty oracle is >= 100 bars from the true one."""
    best = (0.0, None)
    for fx in _fixtures_of(kind):
        ref_loss, _li, ref, _p = T.loss_and_grads(kind, fx.frames, fx.targets, fx.weights, np.float64)
        loss, grads = G.mutant_loss_and_grads(kind, fx.frames, fx.targets, fx.weights, fault)
        ratios = [("loss", abs(loss - ref_loss) / abs(ref_loss) / G.LOSS_BAR)] + [(nm, err / bar) for nm, err, bar in G.grad_errors(kind, grads, ref)]
        for nm, r in ratios:
            if r > best[0]:
                best = (r, f"{fx.shape} {fx.name} {nm}")
    print(f"{kind} {fault}: {best[0]:.3g} bars on {best[1]}")
    assert best[0] >= SEEN, f"no gates fixture sees '{fault}': at most {best[0]:.3g} bars ({best[1]})"


@pytest.mark.parametrize("kind,shape,fault", [("deployed", (3,), "relu_ge_conv"), ("deployed", (10,), "relu_ge_readout"), ("cnnpy", (10, 10, 5), "relu_ge_conv"),
                                              ("cnnpy", (6, 16, 2), "relu_ge_hidden"), ("cnnpy", (5, 1, 16), "relu_ge_hidden")])
def test_a_gate_that_opens_at_zero_fails_the_pure_silent_batch(kind, shape, fault):
    """What the GPU test asserts on the all-silent batch -- exact zeros in front of the last bias-fed layer, the oracle's values
    behind it -- does not survive a `>=`: a tensor that must be 0.0 is not, or a compared one moves by >= 100 bars."""
    fx = G.pure(kind, shape, "silent", 17)
    _l, _li, ref, _p = T.loss_and_grads(kind, fx.frames, fx.targets, fx.weights, np.float64)
    _l, grads = G.mutant_loss_and_grads(kind, fx.frames, fx.targets, fx.weights, fault)
    flat_ref, flat_mut = T.flatten_weights(ref), T.flatten_weights(grads)
    assert all(not np.any(flat_ref[i]) for i in G.SILENT_EXACT_ZERO)      # (conv kernel, conv bias, first dense kernel: both nets)
    broke_a_zero = any(np.any(flat_mut[i]) for i in G.SILENT_EXACT_ZERO)
    moved = max(err / bar for _nm, err, bar in G.grad_errors(kind, grads, ref))
    print(f"{kind} {shape} {fault}: zero broken {broke_a_zero}, largest move {moved:.3g} bars")
    assert broke_a_zero or moved >= SEEN


@pytest.mark.parametrize("kind,shape", [("deployed", (3,)), ("deployed", (10,)), ("cnnpy", (10, 10, 5)), ("cnnpy", (5, 1, 16))])
def test_the_oracle_matches_torch_autograd_on_a_gates_fixture(kind, shape):
    fx = G.mixed(kind, shape, 93)
    x, y = fx.frames.astype(np.float64), fx.targets.astype(np.float64)
    loss, li, grads, p = T.loss_and_grads(kind, x, y, fx.weights, np.float64)
    tw = [(torch.tensor(k, dtype=torch.float64, requires_grad=True), torch.tensor(b, dtype=torch.float64, requires_grad=True)) for k, b in fx.weights]
    tl, tli, tp = _torch_loss(kind, torch.tensor(x), torch.tensor(y), tw)
    tl.backward()
    assert abs(loss - tl.item()) <= 1e-12 * abs(loss)
    np.testing.assert_allclose(li, tli.detach().numpy(), rtol=1e-11, atol=1e-13)
    mem = G.membership(fx)
    clipped = mem["low"]
    assert clipped.sum() >= 4 and np.allclose(li[clipped], -np.log(1e-7), rtol=1e-12)      # the clipped frames' loss term
    for (dk, db), (tk, tb) in zip(grads, tw):
        for g, t in ((dk, tk), (db, tb)):
            ref = t.grad.numpy()
            assert np.abs(ref).max() > 0
            assert np.abs(g - ref).max() <= 1e-10 * np.abs(ref).max()


# ---------------------------------------------------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------------------------------------------------
def _adam_inputs(batch):
    """Weights, f32-oracle gradient and moments for one isolated update on the deployed 3-filter net: batch 'silent' leaves whole
    tensors with a gradient of exactly 0 (the conv kernel there also gets m = v = 0), 'signal' none."""
    fx = G.adam_fixture("deployed", (3,), batch)
    _l, _li, g, _p = T.loss_and_grads(fx.kind, fx.frames, fx.targets, fx.weights, np.float32)
    w, g = T.flatten_weights(fx.weights), [a.astype(np.float32) for a in T.flatten_weights(g)]
    assert all(np.any(a) for a in g) if batch == "signal" else not any(np.any(a) for a in g[:3])
    m, v = G.adam_moments([a.shape for a in w], seed=5, zero=(0,) if batch == "silent" else ())
    return w, g, m, v


@pytest.mark.parametrize("fault", G.ADAM_FAULTS)
def test_every_adam_mutant_is_seen_at_100_bars(fault):
    best = (0.0, None)
    for batch in ("silent", "signal"):
        w, g, m, v = _adam_inputs(batch)
        for case, hyper in G.ADAM_CASES.items():
            for it in G.ADAM_ITERATIONS:
                w1, m1, v1 = G.adam_step(w, g, m, v, it, hyper)
                w2, m2, v2 = G.adam_step(w, g, m, v, it, hyper, fault)
                for i in range(len(w)):
                    bar_m, bar_v, bar_dw = G.adam_bars(m[i], v[i], g[i], w1[i].astype(np.float64) - w[i], it, hyper)
                    with np.errstate(all="ignore"):
                        ratios = {"m": np.abs(m2[i].astype(np.float64) - m1[i]) / np.maximum(bar_m, 1e-300), "v": np.abs(v2[i].astype(np.float64) - v1[i]) / np.maximum(bar_v, 1e-300),
                                  "dw": np.abs(w2[i].astype(np.float64) - w1[i]) / max(bar_dw, 1e-300)}
                    for nm, r in ratios.items():
                        r = float(np.nanmax(np.where(np.isfinite(r), r, 0.0))) if r.size else 0.0      # (t = 0 gives the mutant NaN: not counted)
                        if r > best[0]:
                            best = (r, f"{batch} {case} iterations={it} tensor {i} {nm}")
    print(f"adam {fault}: {best[0]:.3g} bars on {best[1]}")
    assert best[0] >= SEEN, f"no case sees '{fault}': at most {best[0]:.3g} bars ({best[1]})"


def test_the_zero_block_stays_put_and_the_bars_admit_the_oracle_itself():
    """m = v = g = 0: KerasAdam leaves the weight bit-identical (0 / (0 + eps) = 0, no NaN) at every case; and an f64
    evaluation of the same update lies inside the bars (they are not tighter than f32 arithmetic allows)."""
    w, g, m, v = _adam_inputs("silent")
    assert not np.any(g[0]) and not np.any(m[0]) and not np.any(v[0]) and np.any(m[1]) and not np.any(g[1])
    for case, hyper in G.ADAM_CASES.items():
        for it in G.ADAM_ITERATIONS:
            w1, m1, v1 = G.adam_step(w, g, m, v, it, hyper)
            assert np.array_equal(w1[0], w[0]) and not np.any(m1[0]) and not np.any(v1[0])
            t = it + 1
            lr, b1, b2, eps = (float(np.float32(hyper[k])) for k in ("lr", "beta1", "beta2", "eps"))
            alpha = lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t)
            for i in range(len(w)):
                g64, mm, vv = g[i].astype(np.float64), m[i].astype(np.float64), v[i].astype(np.float64)
                m64 = mm + (g64 - mm) * (1 - b1)
                v64 = vv + (g64 * g64 - vv) * (1 - b2)
                dw64 = -(m64 * alpha) / (np.sqrt(v64) + eps)
                bar_m, bar_v, bar_dw = G.adam_bars(m[i], v[i], g[i], w1[i].astype(np.float64) - w[i], it, hyper)
                assert np.all(np.abs(m1[i] - m64) <= bar_m) and np.all(np.abs(v1[i] - v64) <= bar_v), (case, it, i)
                # (w' - w in f32 also carries the rounding of w' itself: half an ulp of the weight, not part of the update's arithmetic)
                assert np.all(np.abs((w1[i].astype(np.float64) - w[i]) - dw64) <= bar_dw + 2.0 ** -24 * np.abs(w[i])), (case, it, i)


@pytest.mark.parametrize("kind,shape", G.ADAM_TOPOLOGIES)
def test_the_bar_on_dw_clears_the_rounding_of_the_weights(kind, shape):
    """w' = fl(w - dw): an ulp of w comes on top of whatever the update computes.  On the Adam fixtures (small weights, one element
    per tensor with v = 0) the bar on dw is at least 4 ulps of the largest weight at every case -- with the oracle's own f32
    gradient here; the GPU test asserts the same with the GPU's before it looks at a result."""
    for batch in ("silent", "signal"):
        fx = G.adam_fixture(kind, shape, batch)
        _l, _li, g, _p = T.loss_and_grads(kind, fx.frames, fx.targets, fx.weights, np.float32)
        w, g = T.flatten_weights(fx.weights), [a.astype(np.float32) for a in T.flatten_weights(g)]
        zero = (0,) if batch == "silent" else ()
        m, v = G.adam_moments([a.shape for a in w], seed=11, zero=zero)
        for case, hyper in G.ADAM_CASES.items():
            for it in G.ADAM_ITERATIONS:
                w1, _m1, _v1 = G.adam_step(w, g, m, v, it, hyper)
                for i in range(len(w)):
                    bar_dw = G.adam_bars(m[i], v[i], g[i], w1[i].astype(np.float64) - w[i], it, hyper)[2]
                    if i in zero or bar_dw == 0.0:      # (beta1 = 0 on a tensor with g == 0: a step of exactly 0)
                        assert np.array_equal(w1[i], w[i])
                        continue
                    assert G.adam_rounding_clearance(w[i], bar_dw) >= 4.0, (batch, case, it, i)
