"""The head trainer (csrc/head_train.hip) on the fixtures of tests/head_gates.py: every tile form and launch plan the kernels have
(head_gates.BRANCHES), both sides of the Keras clip, Dropout rates other than (0.5, 0.5), one Adam update away from its defaults,
the Dropout step key after set_optimizer_state, and a small batch after a larger one on the same trainer.

Bars: the head suite's (tests/test_head_train_gpu.py) -- loss 1e-5 relative, every gradient tensor within 1e-5 of its largest
entry, GPU f32 against the f64 reference of tests/head_train_ref.py; one applied step within 1e-4 of max|w - w0|; exact zeros and
bit-identity are asserted with ==; Adam's bars are train_gates.adam_bars.  tests/test_head_gates.py shows on the CPU that the
reference with any one of the named faults misses these bars by a factor of 100 or more on these very fixtures.

Measured on an MI355X (worst ratio to the bar, printed by the tests): see DESIGN.md section 5.11, "Head gates fixtures"."""
import functools

import numpy as np
import pytest

from modulationdetectioncnn_amd import _cabi
from modulationdetectioncnn_amd.training import HeadTrainer
from tests import head_gates as HG
from tests import head_train_ref as R
from tests import train_gates as G

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _step(tr, f, y, order=None, first=0, count=None, apply=False):
    tr.read()
    tr.train_batch(f, y, order, first, count, apply=apply)
    r = tr.read()
    return r["train_loss_sum"] / max(r["train_rows"], 1), tr.gradients()


def _hold(tag, loss, grads, ref_loss, ref_grads) -> float:
    rs = HG.ratios(loss, grads, ref_loss, ref_grads)
    worst = max(r for _n, r in rs)
    print(f"{tag}: worst ratio to the bar {worst:.3f}  " + " ".join(f"{nm}={r:.3f}" for nm, r in rs))
    for r in R.flat(ref_grads):
        assert np.abs(r).max() > 0
    for nm, r in rs:
        assert r <= 1.0, f"{tag}: {nm} is at {r:.3g} bars"
    return worst


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(R.flat(a), R.flat(b)))


def _through_order(sel, seed=1, first=5):
    """`sel` shuffled, behind `first` positions that are not the batch's: -> (the rows in batch order, order)."""
    sel = np.random.default_rng(seed).permutation(sel)
    return sel, np.concatenate([np.zeros(first, np.int64), sel]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _reference(case):
    """The f64 reference on the case's guarded rows: computed once, shared, never modified.  The direct run and the run through
    `order` take the same rows in another order: one reference serves both (its own sums move by 1e-16 with the order)."""
    fx = R.fixture(*case)
    loss, _li, grads, _p = R.loss_and_grads(fx.f[fx.keep], fx.y[fx.keep], fx.w)
    return loss, grads


# ---- every tile form and launch plan ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", HG.CASES, ids=str)
def test_every_tile_form(case):
    """Loss and the four gradient tensors directly, through `order` with first = 5 and under Dropout (0.5, 0.5) (through `order`:
    the masks are keyed by the row's index in the resident buffer); the evaluation statistics of the same rows; then one applied
    step against the reference's."""
    fx = R.fixture(*case)
    ref_loss, ref_grads = _reference(case)
    fd, yd = _dev(fx.f), _dev(fx.y)
    tr = HeadTrainer(fx.K, fx.H, fx.C, fx.w, device=0, max_batch=fx.count)
    loss, grads = _step(tr, _dev(fx.f[fx.keep]), _dev(fx.y[fx.keep]))
    worst = _hold(f"{case} direct", loss, grads, ref_loss, ref_grads)
    _sel, order = _through_order(fx.keep)
    loss, grads = _step(tr, fd, yd, _dev(order), 5, fx.count)
    worst = max(worst, _hold(f"{case} order", loss, grads, ref_loss, ref_grads))
    assert _same(tr.get_weights(), fx.w) and tr.read()["iterations"] == 0      # nothing was applied
    # the evaluation (launches 1 and 2 as head_row_kernel<false, false>, the statistics of 5) through the same order, on the rows
    # whose two largest probabilities the reference has further apart than f32 could move them
    p2 = np.sort(R.forward(fx.f[_sel], fx.w)["p"], axis=1)
    clear = np.flatnonzero(p2[:, -1] - p2[:, -2] > 1e-4)
    assert len(clear) >= 0.9 * fx.count
    ls, hits = R.evaluate(fx.f[_sel[clear]], fx.y[_sel[clear]], fx.w)
    tr.evaluate_enqueue(fd, yd, _dev(order[5:][clear]))
    r = tr.read()
    print(f"{case} evaluation of {len(clear)} rows: loss sum {r['eval_loss_sum']!r} ref {ls!r}, hits {r['eval_correct']} ref {hits}")
    assert r["eval_rows"] == len(clear) and r["eval_correct"] == hits and abs(r["eval_loss_sum"] - ls) <= HG.LOSS_BAR * ls and r["train_rows"] == 0
    td = HeadTrainer(fx.K, fx.H, fx.C, fx.w, device=0, max_batch=fx.count, dropout=fx.dropout["rates"], dropout_seed=fx.dropout["seed"])
    sel, order = _through_order(fx.keep_drop)
    loss, grads = _step(td, fd, yd, _dev(order), 5, fx.count)
    dl, _li, dg, _p = R.loss_and_grads(fx.f[sel], fx.y[sel], fx.w, np.float64, dict(fx.dropout, frames=sel))
    assert R.rel(dg[0][0], ref_grads[0][0]) > 100 * HG.GRAD_BAR                 # the masks act: a step that ignored them would miss dW1's bar 100 times over
    worst = max(worst, _hold(f"{case} dropout", loss, grads, dl, dg))
    # one applied step
    w = [(k.copy(), b.copy()) for k, b in fx.w]
    R.KerasAdam([t.shape for t in R.flat(w)]).apply(R.flat(w), R.flat(ref_grads))      # (R.train_step on the reference's gradients)
    tr.train_batch(_dev(fx.f[fx.keep]), _dev(fx.y[fx.keep]))
    assert tr.read()["iterations"] == 1
    errs = [float(np.abs(a.astype(np.float64) - b).max()) / max(float(np.abs(b.astype(np.float64) - c).max()), 1e-30)
            for a, b, c in zip(R.flat(tr.get_weights()), R.flat(w), R.flat(fx.w))]
    print(f"{case} one step: error / max|w - w0| per tensor, in bars of {HG.STEP_BAR:g}:", [e / HG.STEP_BAR for e in errs], "gradients' worst", worst)
    assert max(errs) <= HG.STEP_BAR, errs


# ---- the clip --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", HG.CLIP_SHAPES, ids=str)
def test_mixed_clip_batch(shape):
    """Interior rows, rows clipped below and above, label-smoothed rows, rows summing to 2 and to 0, and smoothed rows with one
    class clipped beside a passing one, interleaved in one batch of 93: directly and through a shuffle."""
    fx = HG.mixed(*shape)
    HG.check_preconditions(fx)      # (an AssertionError here is a broken fixture: an error, not a skip)
    ref_loss, _li, ref_grads, _p = R.loss_and_grads(fx.f, fx.y, fx.weights)
    tr = HeadTrainer(fx.K, fx.H, fx.C, fx.weights, device=0, max_batch=len(fx.f))
    loss, grads = _step(tr, _dev(fx.f), _dev(fx.y))
    _hold(f"clip {shape} {fx.name}", loss, grads, ref_loss, ref_grads)
    fr, yr, order, first = HG.shuffled(fx)
    loss, grads = _step(tr, _dev(fr), _dev(yr), _dev(order), first, len(fx.f))
    _hold(f"clip {shape} {fx.name} shuffled", loss, grads, ref_loss, ref_grads)


@pytest.mark.parametrize("n", HG.PURE_COUNTS)
@pytest.mark.parametrize("category", HG.PURE_KINDS)
@pytest.mark.parametrize("shape", HG.CLIP_SHAPES, ids=str)
def test_pure_clipped_batches_are_exact(shape, category, n):
    """Every row clipped on one side: EVERY gradient element is 0.0, the loss is the f32 reference's (n x -log 1e-7 below,
    -log(1 - 1e-7) as f32 has it above), and the evaluation of the same rows gives that loss and the reference's hit count."""
    fx = HG.pure(*shape, category, n)
    HG.check_preconditions(fx)
    tr = HeadTrainer(fx.K, fx.H, fx.C, fx.weights, device=0, max_batch=n)
    fd, yd = _dev(fx.f), _dev(fx.y)
    loss, grads = _step(tr, fd, yd)
    for i, g in enumerate(R.flat(grads)):
        assert np.all(g == 0.0), f"tensor {i}: {np.count_nonzero(g)} elements of an all-'{category}' batch's gradient are not 0"
    loss32 = R.loss_and_grads(fx.f, fx.y, fx.weights, np.float32)[0]
    ls32, _h = R.evaluate(fx.f, fx.y, fx.weights, np.float32)
    _ls, hits = R.evaluate(fx.f, fx.y, fx.weights)
    tr.evaluate_enqueue(fd, yd)
    r = tr.read()
    print(f"clip {shape} {fx.name}: loss {loss!r}, f32 reference {loss32!r}; evaluation {r['eval_loss_sum']!r} / {r['eval_correct']}, reference {ls32!r} / {hits}")
    assert abs(loss - loss32) <= 1e-6 * abs(loss32)
    assert hits == (n if category == "high" else 0)
    assert r["eval_rows"] == n and r["eval_correct"] == hits and abs(r["eval_loss_sum"] - ls32) <= 1e-6 * abs(ls32)


# ---- Dropout ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rates", HG.RATE_PAIRS, ids=str)
@pytest.mark.parametrize("shape", HG.RATE_SHAPES, ids=str)
def test_dropout_rate_pairs(shape, rates):
    """One site only (the mixed template pairs z1<., true> + row<true, false> and z1<., false> + row<true, true>), rates whose
    1 / (1 - rate) is no power of two, nine features in ten dropped: against the reference with the same generator, on rows the
    guard keeps under that mask."""
    fx = R.fixture(*shape)
    kept, drop = HG.keep_under(fx, rates)
    sel, order = _through_order(kept)
    tr = HeadTrainer(fx.K, fx.H, fx.C, fx.w, device=0, max_batch=fx.count, dropout=rates, dropout_seed=drop["seed"])
    loss, grads = _step(tr, _dev(fx.f), _dev(fx.y), _dev(order), 5, fx.count)
    ref_loss, _li, ref_grads, _p = R.loss_and_grads(fx.f[sel], fx.y[sel], fx.w, np.float64, dict(drop, frames=sel))
    _hold(f"{shape} rates {rates}", loss, grads, ref_loss, ref_grads)


def test_skipped_positions_under_dropout():
    """The out-of-range-index case of tests/test_head_train_gpu.py under Dropout (0.5, 0.5): the two positions that name no row
    contribute nothing, and the mean still divides by `count`."""
    fx = R.fixture(*HG.SKIP_SHAPE)
    sel = fx.keep_drop
    order = HG.skip_order(fx, sel)
    tr = HeadTrainer(fx.K, fx.H, fx.C, fx.w, device=0, max_batch=32, dropout=fx.dropout["rates"], dropout_seed=fx.dropout["seed"])
    tr.read()
    tr.train_batch(_dev(fx.f), _dev(fx.y), _dev(order), 0, len(order), apply=False)
    with pytest.raises(_cabi.MdcError, match="2 batch positions") as e:
        tr.read()
    assert e.value.code == -22
    _l, _li, ref_grads, _p = R.loss_and_grads(fx.f[sel], fx.y[sel], fx.w, np.float64, dict(fx.dropout, frames=sel), divide_by=len(order))
    errs = [R.rel(g, r) / HG.GRAD_BAR for g, r in zip(R.flat(tr.gradients()), R.flat(ref_grads))]
    print("skipped positions under Dropout: dW1 db1 dW2 db2 in bars", errs)
    assert max(errs) <= 1.0, errs


def test_dropout_step_follows_set_iterations():
    """The Dropout step key reads `iterations` from the device: after set_optimizer_state(iterations=950) a batch is masked as the
    reference's step 950 -- on rows the guard keeps under THAT mask -- and not as step 0."""
    fx = R.fixture(*HG.STEP_SHAPE)
    kept, drop = HG.keep_under(fx, (0.5, 0.5), step=HG.STEP_ITERATIONS)
    sel, order = _through_order(kept)
    tr = HeadTrainer(fx.K, fx.H, fx.C, fx.w, device=0, max_batch=fx.count, dropout=(0.5, 0.5), dropout_seed=drop["seed"])
    zeros = [(np.zeros_like(k), np.zeros_like(b)) for k, b in fx.w]
    tr.set_optimizer_state({"iterations": HG.STEP_ITERATIONS, "m": zeros, "v": zeros})
    loss, grads = _step(tr, _dev(fx.f), _dev(fx.y), _dev(order), 5, fx.count)
    assert tr.read()["iterations"] == HG.STEP_ITERATIONS
    ref_loss, _li, ref_grads, _p = R.loss_and_grads(fx.f[sel], fx.y[sel], fx.w, np.float64, dict(drop, frames=sel))
    _hold(f"{HG.STEP_SHAPE} Dropout at step {HG.STEP_ITERATIONS}", loss, grads, ref_loss, ref_grads)
    loss0 = R.loss_and_grads(fx.f[sel], fx.y[sel], fx.w, np.float64, dict(drop, frames=sel, step=0))[0]
    assert abs(loss - loss0) > 1e-3 * abs(loss), (loss, loss0)


# ---- Adam ------------------------------------------------------------------------------------------------------------------------
def _pairs(flat):
    return list(zip(flat[0::2], flat[1::2]))


@pytest.mark.parametrize("case", list(G.ADAM_CASES))
@pytest.mark.parametrize("shape", HG.ADAM_SHAPES, ids=str)
def test_one_adam_update_isolated_from_the_gradient(shape, case):
    """tests/test_train_gates_gpu.py's test of this name on HeadTrainer: set w, m, v and `iterations`; read the batch's gradient g
    with apply=False; run the batch again with apply=True; feed that g with what was set to KerasAdam (f32).  m' and v'
    element-wise, w' - w relative to the reference's largest step (train_gates.adam_bars).  On the all-zero batch dW1's gradient
    is exactly 0 and W1 has m = v = 0: it must come back bit-identical.  W1 goes through head_adam_kernel's float4 half, b1, W2
    and b2 through its scalar tail."""
    hyper = G.ADAM_CASES[case]
    worst = {"m": 0.0, "v": 0.0, "dw": 0.0}
    tr = None
    for batch in ("zero", "signal"):
        w0, f, y = HG.adam_fixture(*shape, batch)
        w = R.flat(w0)
        zero = (0,) if batch == "zero" else ()
        m, v = G.adam_moments([a.shape for a in w], seed=11, zero=zero)
        if tr is None:
            tr = HeadTrainer(*shape, w0, device=0, max_batch=len(f), **hyper)
        fd, yd = _dev(f), _dev(y)
        for it in G.ADAM_ITERATIONS:
            tr.set_weights(w0)
            tr.set_optimizer_state({"iterations": it, "m": _pairs(m), "v": _pairs(v)})
            tr.train_batch(fd, yd, apply=False)
            g = R.flat(tr.gradients())
            assert tr.read()["iterations"] == it
            assert all(np.any(a) for a in g[1:]) and (np.all(g[0] == 0.0) if batch == "zero" else np.any(g[0]))
            tr.train_batch(fd, yd, apply=True)
            got_w, st = R.flat(tr.get_weights()), tr.optimizer_state()
            got_m, got_v = R.flat(st["m"]), R.flat(st["v"])
            assert st["iterations"] == it + 1
            ref_w, ref_m, ref_v = G.adam_step(w, g, m, v, it, hyper)
            for i in range(len(w)):
                assert np.isfinite(got_w[i]).all() and np.isfinite(got_m[i]).all() and np.isfinite(got_v[i]).all()
                dw_ref = ref_w[i].astype(np.float64) - w[i]
                bar_m, bar_v, bar_dw = G.adam_bars(m[i], v[i], g[i], dw_ref, it, hyper)
                if i in zero:
                    assert np.array_equal(got_w[i].view(np.uint32), w[i].view(np.uint32)) and not np.any(got_m[i]) and not np.any(got_v[i])
                    continue
                # fixture check: w' = fl(w - dw) carries up to an ulp of w whatever the update computes; it must stay well inside the bar
                assert bar_dw > 0 and G.adam_rounding_clearance(w[i], bar_dw) >= 4.0, f"{batch} {it} tensor {i}: the bar on dw ({bar_dw:.3g}) does not clear the weights' rounding"
                em, ev = np.abs(got_m[i].astype(np.float64) - ref_m[i]), np.abs(got_v[i].astype(np.float64) - ref_v[i])
                edw = np.abs((got_w[i].astype(np.float64) - w[i]) - dw_ref).max()
                with np.errstate(all="ignore"):
                    rm = float(np.max(np.where(em > 0, em / bar_m, 0.0)))
                    rv = float(np.max(np.where(ev > 0, ev / bar_v, 0.0)))
                worst = {"m": max(worst["m"], rm), "v": max(worst["v"], rv), "dw": max(worst["dw"], edw / bar_dw)}
                assert rm <= 1.0 and rv <= 1.0 and edw <= bar_dw, f"{batch} iterations={it} tensor {i}: m {rm:.3g} v {rv:.3g} dw {edw / bar_dw:.3g} bars"
    print(f"adam head {shape} {case}: worst ratio to the bar  m' {worst['m']:.3f}  v' {worst['v']:.3f}  dw {worst['dw']:.3f}")


# ---- stale scratch ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,counts", [((10560, 256, 11, 257), (257, 1, 97)), ((64, 224, 5, 9400), (9400, 70))], ids=str)
def test_a_small_batch_after_a_large_one_is_bit_identical_to_a_fresh_trainer(shape, counts):
    """The scratch keeps what the larger batch wrote (K-slice partials of more row tiles, partial dW1 of more batch slices, more
    launch-4 slices): a launch that read a partial it did not write THIS step would differ from a trainer that never saw it."""
    fx = R.fixture(*shape)
    fd, yd = _dev(fx.f), _dev(fx.y)
    tr = HeadTrainer(fx.K, fx.H, fx.C, fx.w, device=0, max_batch=counts[0])
    for n in counts:
        order = _dev(fx.keep[:n].astype(np.int32))
        loss, grads = _step(tr, fd, yd, order, 0, n)
        fresh = HeadTrainer(fx.K, fx.H, fx.C, fx.w, device=0, max_batch=n)
        fl, fg = _step(fresh, fd, yd, order, 0, n)
        assert loss == fl and _same(grads, fg), f"count {n} after {counts[:counts.index(n)]}"
        assert all(np.abs(g).max() > 0 for g in R.flat(grads))
