"""The training kernels (csrc/train.hip) on the gates fixtures of tests/train_gates.py: every branch of the clip, of the three
ReLU gates, of the per-class target masks and of cnn.py's padded tiles, and one Adam update away from its defaults.

Bars: the project's own for the backward pass (tests/test_training_gpu.py) -- loss 1e-5 relative, kernel gradients 1e-5 and
bias gradients 2e-5 of the tensor's largest entry, GPU f32 against the f64 oracle; exact zeros are asserted with ==; Adam's
bars are derived in train_gates.adam_bars.  tests/test_train_gates.py shows on the CPU that an oracle with any one of the
named faults misses these bars by a factor of 100 or more on these very batches.

Measured on an MI355X (worst ratio to the bar, printed by the tests): see DESIGN.md section 5.11."""
import functools
import math

import numpy as np
import pytest

from modulationdetectioncnn_amd import VTCNN2
from modulationdetectioncnn_amd.training import Trainer
from oracle import oracle_train as T
from tests import train_gates as G

pytestmark = pytest.mark.gpu

CASES = [(k, s, n) for k, s in G.TOPOLOGIES for n in G.MIXED_COUNTS]
CASE_IDS = [f"{i}-{n}" for i in G.TOPOLOGY_IDS for n in G.MIXED_COUNTS]


@functools.lru_cache(maxsize=None)
def _fixture(kind, shape, n):
    """The mixed batch, its preconditions checked (an AssertionError here is a broken fixture: an error, not a skip), and the f64
    oracle on it: computed once, shared by the tests below, never modified."""
    fx = G.mixed(kind, shape, n)
    G.check_preconditions(fx)
    loss, _li, grads, _p = T.loss_and_grads(kind, fx.frames, fx.targets, fx.weights, np.float64)
    return fx, loss, grads


def _hold(tag, kind, loss, grads, ref_loss, ref_grads):
    ratios = [("loss", abs(loss - ref_loss) / abs(ref_loss) / G.LOSS_BAR)] + [(nm, err / bar) for nm, err, bar in G.grad_errors(kind, grads, ref_grads)]
    print(f"{tag}: worst ratio to the bar {max(r for _n, r in ratios):.3f}  " + " ".join(f"{nm}={r:.3f}" for nm, r in ratios))
    for nm, r in ratios:
        assert r <= 1.0, f"{tag}: {nm} is at {r:.3g} bars"


def _through_the_shuffle(tr, fx):
    import torch
    xr, yr, order, first = G.shuffled(fx)
    n = len(fx.frames)
    tr.read(reset=True)
    tr.train_batch(tr._frames(xr), tr._targets(yr, n), torch.from_numpy(order).cuda(), first, n, apply=False)
    r = tr.read(reset=True)
    assert r["train_frames"] == n
    return r["train_loss_sum"] / n, tr.gradients(), order[first:]


@pytest.mark.parametrize("kind,shape,n", CASES, ids=CASE_IDS)
def test_mixed_gates_batch(kind, shape, n):
    """Interior, clipped-low, clipped-high, silent, dead and soft-target frames interleaved in one ragged batch: loss and every
    gradient against the f64 oracle -- directly, addressed through a shuffle (first != 0), and under Dropout 0.5."""
    fx, ref_loss, ref_grads = _fixture(kind, shape, n)
    tr = Trainer(fx.topology, fx.weights, device=0)
    loss, grads = tr.loss_and_gradients(fx.frames, fx.targets)
    _hold(f"{kind}{shape} n={n}", kind, loss, grads, ref_loss, ref_grads)
    loss_s, grads_s, _frames = _through_the_shuffle(tr, fx)
    _hold(f"{kind}{shape} n={n} shuffled", kind, loss_s, grads_s, ref_loss, ref_grads)
    for (k, b), (k0, b0) in zip(tr.get_weights(), fx.weights):      # nothing was applied
        assert np.array_equal(k, k0) and np.array_equal(b, b0)
    seed = G.dropout_seed(fx)
    td = Trainer(fx.topology, fx.weights, device=0, dropout=G.DROPOUT_RATE, dropout_seed=seed)
    loss_d, grads_d, frames = _through_the_shuffle(td, fx)
    dl, _li, dg, _p = T.loss_and_grads(kind, fx.frames, fx.targets, fx.weights, np.float64,
                                       dropout=dict(rate=G.DROPOUT_RATE, seed=seed, step=0, frames=frames))
    assert abs(dl - ref_loss) > 1e-3 * ref_loss                     # the masks act
    _hold(f"{kind}{shape} n={n} dropout seed {seed}", kind, loss_d, grads_d, dl, dg)


PURE = [(k, s, c, n) for k, s in G.TOPOLOGIES for c in G.PURE_KINDS if c != "dead" or k == "deployed" for n in G.PURE_COUNTS]
PURE_IDS = [f"{i}-{c}-{n}" for (k, s), i in zip(G.TOPOLOGIES, G.TOPOLOGY_IDS) for c in G.PURE_KINDS if c != "dead" or k == "deployed" for n in G.PURE_COUNTS]


@pytest.mark.parametrize("kind,shape,category,n", PURE, ids=PURE_IDS)
def test_pure_batches_are_exact(kind, shape, category, n):
    """All frames clipped (either side) or all read-outs dead: EVERY gradient element is 0.0 and the loss is the f32 oracle's
    (log 3 for the dead read-out).  All frames silent under a zero conv bias: the conv kernel, the conv bias and the first dense
    kernel have a gradient of exactly 0 (every conv gate sits on 0 and must block); what the biases feed matches the oracle."""
    fx = G.pure(kind, shape, category, n)
    G.check_preconditions(fx)
    loss, grads = Trainer(fx.topology, fx.weights, device=0).loss_and_gradients(fx.frames, fx.targets)
    flat = T.flatten_weights(grads)
    assert all(np.isfinite(g).all() for g in flat)
    if category == "silent":
        for i in G.SILENT_EXACT_ZERO:
            assert np.all(flat[i] == 0.0), f"tensor {i}: {np.count_nonzero(flat[i])} elements of the silent batch's gradient are not 0"
        ref_loss, _li, ref_grads, _p = T.loss_and_grads(kind, fx.frames, fx.targets, fx.weights, np.float64)
        assert np.any(T.flatten_weights(ref_grads)[-1])
        _hold(f"{kind}{shape} {fx.name}", kind, loss, grads, ref_loss, ref_grads)
        return
    for i, g in enumerate(flat):
        assert np.all(g == 0.0), f"tensor {i}: {np.count_nonzero(g)} elements of an all-'{category}' batch's gradient are not 0"
    loss32, _li, _g, _p = T.loss_and_grads(kind, fx.frames, fx.targets, fx.weights, np.float32)
    print(f"{kind}{shape} {fx.name}: loss {loss!r}, f32 oracle {loss32!r}")
    assert abs(loss - loss32) <= 1e-6 * abs(loss32)
    if category == "dead":
        assert abs(loss - math.log(3.0)) <= 1e-6 * math.log(3.0)


@pytest.mark.parametrize("kind,shape,n", CASES, ids=CASE_IDS)
def test_both_evaluate_paths_on_the_one_hot_frames(kind, shape, n):
    """Trainer.evaluate (the training kernels' forward) and VTCNN2.evaluate (mdc_forward + mdc_crossentropy) against the oracle
    on the fixture's one-hot frames, and against each other on its clipped frames alone."""
    fx, _l, _g = _fixture(kind, shape, n)
    mem = G.membership(fx)
    tr = Trainer(fx.topology, fx.weights, device=0)
    m = VTCNN2(fx.topology, device=0)
    m.set_weights(fx.weights)
    hot = G._is_onehot(fx.targets.astype(np.float64))
    for name, sel in (("one-hot", hot), ("clipped", mem["low"] | mem["high"]), ("clipped-low", mem["low"])):
        x, y = fx.frames[sel], fx.targets[sel]
        assert len(x) >= G.MIN_PER_CATEGORY
        ref = T.evaluate(kind, x, y, fx.weights, np.float64)
        a, b = tr.evaluate(x, y), m.evaluate(x, y)
        print(f"{kind}{shape} n={n} {name}: oracle {ref!r} trainer {a!r} inference {b!r}")
        assert abs(a - ref) <= 1e-5 * ref and abs(b - ref) <= 1e-5 * ref and abs(a - b) <= 1e-5 * ref
    x, y = fx.frames[mem["high"]], fx.targets[mem["high"]]          # all above the clip: -log(1 - 1e-7) as f32 has it, in both paths
    ref32 = T.evaluate(kind, x, y, fx.weights, np.float32)
    a, b = tr.evaluate(x, y), m.evaluate(x, y)
    assert abs(a - ref32) <= 1e-5 * ref32 and abs(b - ref32) <= 1e-5 * ref32, (a, b, ref32)


ADAM_TOPOLOGIES = G.ADAM_TOPOLOGIES


def _pairs(flat):
    return list(zip(flat[0::2], flat[1::2]))


@pytest.mark.parametrize("case", list(G.ADAM_CASES))
@pytest.mark.parametrize("kind,shape", ADAM_TOPOLOGIES, ids=["T1-F3", "T2-F10", "T4-10-10-5", "T4-6-16-2"])
def test_one_adam_update_isolated_from_the_gradient(kind, shape, case):
    """Set w, m, v and `iterations`; read the batch's gradient g with apply=False; run the batch again with apply=True; feed that
    g with what was set to KerasAdam (f32).  m' and v' element-wise, w' - w relative to the oracle's largest step (adam_bars).
    On the silent batch whole tensors have g == 0 exactly; the conv kernel there also has m = v = 0: its weights must come back
    bit-identical (0 / (0 + eps), not NaN).  iterations in {0, 1, 950, 100000}."""
    hyper = G.ADAM_CASES[case]
    worst = {"m": 0.0, "v": 0.0, "dw": 0.0}
    tr = None
    for batch in ("silent", "signal"):
        fx = G.adam_fixture(kind, shape, batch)
        w = T.flatten_weights(fx.weights)
        zero = (0,) if batch == "silent" else ()
        m, v = G.adam_moments([a.shape for a in w], seed=11, zero=zero)
        if tr is None:
            tr = Trainer(fx.topology, fx.weights, device=0, **hyper)
        xd, yd = tr._frames(fx.frames), tr._targets(fx.targets, len(fx.frames))
        for it in G.ADAM_ITERATIONS:
            tr.set_weights(fx.weights)
            tr.set_optimizer_state({"iterations": it, "m": _pairs(m), "v": _pairs(v)})
            tr.train_batch(xd, yd, apply=False)
            g = T.flatten_weights(tr.gradients())
            assert tr.read()["iterations"] == it
            if batch == "silent":
                assert all(np.all(g[i] == 0.0) for i in G.SILENT_EXACT_ZERO) and np.any(g[-1])
            else:
                assert all(np.any(a) for a in g)
            tr.train_batch(xd, yd, apply=True)
            got_w, st = T.flatten_weights(tr.get_weights()), tr.optimizer_state()
            got_m, got_v = T.flatten_weights(st["m"]), T.flatten_weights(st["v"])
            assert st["iterations"] == it + 1
            ref_w, ref_m, ref_v = G.adam_step(w, g, m, v, it, hyper)
            for i in range(len(w)):
                assert np.isfinite(got_w[i]).all() and np.isfinite(got_m[i]).all() and np.isfinite(got_v[i]).all()
                dw_ref = ref_w[i].astype(np.float64) - w[i]
                bar_m, bar_v, bar_dw = G.adam_bars(m[i], v[i], g[i], dw_ref, it, hyper)
                if i in zero:
                    assert np.array_equal(got_w[i].view(np.uint32), w[i].view(np.uint32)) and not np.any(got_m[i]) and not np.any(got_v[i])
                    continue
                if bar_dw == 0.0:      # beta1 = 0 on a tensor with g == 0: m' = g = 0, the oracle's step is exactly 0 -- and so must this one be
                    assert np.array_equal(got_w[i], w[i]) and not np.any(got_m[i]), f"{batch} iterations={it} tensor {i}: a zero step moved the weights"
                    bar_dw = np.inf
                # fixture check: w' = fl(w - dw) carries up to an ulp of w whatever the update computes; it must stay well inside the bar
                assert G.adam_rounding_clearance(w[i], bar_dw) >= 4.0, f"{batch} {it} tensor {i}: the bar on dw ({bar_dw:.3g}) does not clear the weights' rounding"
                em, ev = np.abs(got_m[i].astype(np.float64) - ref_m[i]), np.abs(got_v[i].astype(np.float64) - ref_v[i])
                edw = np.abs((got_w[i].astype(np.float64) - w[i]) - dw_ref).max()
                with np.errstate(all="ignore"):
                    rm = float(np.max(np.where(em > 0, em / bar_m, 0.0)))
                    rv = float(np.max(np.where(ev > 0, ev / bar_v, 0.0)))
                worst = {"m": max(worst["m"], rm), "v": max(worst["v"], rv), "dw": max(worst["dw"], edw / bar_dw)}
                assert rm <= 1.0 and rv <= 1.0 and edw <= bar_dw, f"{batch} iterations={it} tensor {i}: m {rm:.3g} v {rv:.3g} dw {edw / bar_dw:.3g} bars"
    print(f"adam {kind}{shape} {case}: worst ratio to the bar  m' {worst['m']:.3f}  v' {worst['v']:.3f}  dw {worst['dw']:.3f}")
