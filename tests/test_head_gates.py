"""The head gates fixtures of tests/head_gates.py, on the CPU: the plan restatement reads the kernel's own constants and the case
list reaches every named branch of the launch plans; every fixture meets its preconditions on the f64 reference (and its f32
restatement stays within a quarter of the GPU bars); every mutant -- the reference with ONE named fault a tile, a slice or the
clip could have -- leaves the reference by at least 100x the bar tests/test_head_gates_gpu.py applies on some fixture of the
list (a pure clipped batch's bar is `== 0.0`: there a mutant is seen where it turns an exact zero into a number)."""
import numpy as np
import pytest

from tests import head_gates as HG
from tests import head_train_ref as R
from tests import train_gates as G

SEEN = 100.0


# ---- the plan -----------------------------------------------------------------------------------------------------------------
def test_the_plan_restates_the_figures_the_design_states():
    assert HG.kernel_constants() == dict(kHeadBM=128, kHeadBK=32, kHeadTarget=512, kHeadMaxSlices2=4, kSmallSlices=256, kSmallRows=16)
    p = HG.plan(10560, 256, 1024)      # 8 x 2 tiles x 30 K-slices of 11 chunks; 83 x 2 x 3; 64 small slices; 256 x 4 waves
    assert (p["tiles_m"], p["tiles_n"], p["slices"], p["chunks_per"], p["slices2"], p["small"], p["row_grid"]) == (8, 2, 30, 11, 3, 64, 256)
    for count, slices2 in ((96, 3), (128, 2), (65, 3), (1, 1)):      # "96 rows are three one-stage slices, 128 rows two two-stage ones"
        assert HG.plan(10560, 256, count)["slices2"] == slices2
    p = HG.plan(64, 224, 9400)
    assert (p["tiles"], p["s_raw"], p["row_passes"], p["per"], p["empty_small"], p["slices2"], p["rows_per2"]) == (518, 0, 3, 37, 1, 4, 74 * 32)
    p = HG.plan(32, 128, 4097)
    assert (p["row_passes"], p["per"], p["empty_small"]) == (2, 17, 15) and 4097 - 4 * p["row_grid"] == 1
    p = HG.plan(16384, 224, 40)
    assert (p["slices"], p["chunks_per"], p["s2_raw"], p["slices2"]) == (64, 8, 0, 1)
    assert HG.plan(96, 160, 97)["last_rows2"] == 1 and HG.plan(64, 64, 225)["last_rows2"] == 33 and HG.plan(128, 192, 140)["last_rows2"] == 12


def test_the_case_list_reaches_every_named_branch():
    assert HG.missing_branches(HG.CASES + R.SHAPES) == []
    # ... and the list is not reached by accident: the shapes of the head suite alone miss most of it, any big case is needed
    alone = HG.missing_branches(R.SHAPES)
    assert len(alone) >= 15 and "BN 64, one hidden tile" in alone and "two row passes" in alone, alone
    assert "s_raw = 0" in HG.missing_branches([c for c in HG.CASES if c != (64, 224, 5, 9400)] + R.SHAPES)
    assert "s2_raw = 0" in HG.missing_branches([c for c in HG.CASES if c != (16384, 224, 16, 40)] + R.SHAPES)
    for K, H, _C, n in HG.CASES + R.SHAPES:      # every plan fits what mdc_head_trainer_create allocates for max_batch = count
        p = HG.plan(K, H, n)
        assert p["slices"] * p["tiles"] <= max(HG.kernel_constants()["kHeadTarget"], p["tiles"]) and 1 <= p["slices2"] <= min(4, p["stages"])
        assert (p["slices"] - 1) * p["chunks_per"] < p["chunks"] and (p["slices2"] - 1) * p["rows_per2"] < n


# ---- fixtures -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", HG.CASES, ids=str)
def test_every_tile_form_fixture_meets_its_preconditions(case):
    HG.check_preconditions(R.fixture(*case))


@pytest.mark.parametrize("shape", HG.CLIP_SHAPES, ids=str)
def test_every_clip_fixture_meets_its_preconditions(shape):
    fx = HG.mixed(*shape)
    counts = HG.check_preconditions(fx)
    print(shape, counts)
    assert len(fx.f) == HG.MIXED_COUNT and all(counts[c] >= G.MIN_PER_CATEGORY for c in HG.CATEGORIES if c != "partly" or shape[2] >= 3)
    for category in HG.PURE_KINDS:
        for n in HG.PURE_COUNTS:
            assert HG.check_preconditions(HG.pure(*shape, category, n))[category] == n
    fr, yr, order, first = HG.shuffled(fx)
    assert first != 0 and np.array_equal(fr[order[first:]], fx.f) and np.array_equal(yr[order[first:]], fx.y)
    assert not np.array_equal(order[first:], np.arange(len(fx.f)))


def test_a_broken_clip_fixture_is_an_error():
    fx = HG.mixed(96, 32, 3)
    hot = fx.y.copy()
    hot[~HG._is_onehot(hot.astype(np.float64))] = [1, 0, 0]
    with pytest.raises(AssertionError, match="'soft' rows"):
        HG.check_preconditions(HG.ClipBatch(fx.K, fx.H, fx.C, "no-soft", fx.weights, fx.f, hot))
    with pytest.raises(AssertionError, match="not every row"):
        HG.check_preconditions(HG.ClipBatch(fx.K, fx.H, fx.C, "not-pure", fx.weights, fx.f, fx.y, pure="low"))
    grey = [fx.weights[0], ((fx.weights[1][0] * np.float32(0.5)).astype(np.float32), fx.weights[1][1])]      # half the scale: saturated rows fall back into the grey zones
    with pytest.raises(AssertionError, match="grey zone"):
        HG.check_preconditions(HG.ClipBatch(fx.K, fx.H, fx.C, "grey", grey, fx.f, fx.y))


@pytest.mark.parametrize("shape", HG.RATE_SHAPES, ids=str)
@pytest.mark.parametrize("rates", HG.RATE_PAIRS, ids=str)
def test_the_dropout_pair_fixtures_are_well_conditioned(shape, rates):
    fx = R.fixture(*shape)
    sel, drop = HG.keep_under(fx, rates)
    assert len(sel) == fx.count
    faults = HG.restatement_faults(fx.f[sel], fx.y[sel], fx.w, dict(drop, frames=sel))
    assert not faults, faults
    plain = R.loss_and_grads(fx.f[sel], fx.y[sel], fx.w)[0]
    assert abs(R.loss_and_grads(fx.f[sel], fx.y[sel], fx.w, dropout=dict(drop, frames=sel))[0] - plain) > 1e-4 * plain      # the masks act


def test_the_skipped_row_and_the_set_iterations_fixtures_are_well_conditioned():
    fx = R.fixture(*HG.SKIP_SHAPE)
    sel = fx.keep_drop
    order = HG.skip_order(fx, sel)
    assert len(order) == fx.count + 2 and ((order < 0) | (order >= fx.pool)).sum() == 2
    assert not HG.restatement_faults(fx.f[sel], fx.y[sel], fx.w, dict(fx.dropout, frames=sel), divide_by=len(order))
    fx = R.fixture(*HG.STEP_SHAPE)
    sel, drop = HG.keep_under(fx, (0.5, 0.5), step=HG.STEP_ITERATIONS)
    assert drop["step"] == 950 and not HG.restatement_faults(fx.f[sel], fx.y[sel], fx.w, dict(drop, frames=sel))
    at950 = R.loss_and_grads(fx.f[sel], fx.y[sel], fx.w, dropout=dict(drop, frames=sel))[0]
    at0 = R.loss_and_grads(fx.f[sel], fx.y[sel], fx.w, dropout=dict(drop, frames=sel, step=0))[0]
    assert abs(at950 - at0) > 1e-3 * at950      # what the GPU test tells the two steps apart by


# ---- mutants ------------------------------------------------------------------------------------------------------------------
def _scenarios():
    """(name, rows, targets, weights, Dropout, divide_by) of the GPU tests' comparisons, the cheap ones first."""
    for shape in HG.CLIP_SHAPES:
        fx = HG.mixed(*shape)
        yield f"clip {shape} {fx.name}", fx.f, fx.y, fx.weights, None, None
    fx = R.fixture(*HG.SKIP_SHAPE)
    sel = fx.keep_drop
    yield f"skipped rows {HG.SKIP_SHAPE}", fx.f[sel], fx.y[sel], fx.w, dict(fx.dropout, frames=sel), fx.count + 2
    fx = R.fixture(*HG.RATE_SHAPES[0])
    for rates in HG.RATE_PAIRS:
        sel, drop = HG.keep_under(fx, rates)
        yield f"rates {rates} {HG.RATE_SHAPES[0]}", fx.f[sel], fx.y[sel], fx.w, dict(drop, frames=sel), None
    for case in sorted(HG.CASES, key=lambda c: c[0] * c[1] * c[3]):
        fx = R.fixture(*case)
        yield f"tile form {case}", fx.f[fx.keep], fx.y[fx.keep], fx.w, None, None


def test_the_mutant_without_a_fault_is_the_reference():
    fx = R.fixture(*HG.SKIP_SHAPE)
    sel = fx.keep_drop
    for drop, div in ((None, None), (dict(fx.dropout, frames=sel), fx.count + 2)):
        for dtype in (np.float64, np.float32):
            loss, grads = HG.mutant_loss_and_grads(fx.f[sel], fx.y[sel], fx.w, None, dtype, drop, div)
            ref_loss, _li, ref, _p = R.loss_and_grads(fx.f[sel], fx.y[sel], fx.w, dtype, drop, div)
            assert loss == ref_loss and all(np.array_equal(a, b) for a, b in zip(R.flat(grads), R.flat(ref)))


@pytest.mark.parametrize("fault", [f for f in HG.FAULTS if f != "clip_ignored_high"])
def test_every_mutant_is_seen_at_100_bars(fault):
    best = (0.0, None)
    for name, f, y, w, drop, div in _scenarios():
        ref_loss, _li, ref, _p = R.loss_and_grads(f, y, w, np.float64, drop, div)
        loss, grads = HG.mutant_loss_and_grads(f, y, w, fault, np.float64, drop, div)
        for nm, r in HG.ratios(loss, grads, ref_loss, ref):
            if r > best[0]:
                best = (r, f"{name} {nm}")
        if best[0] >= SEEN:
            break
    print(f"{fault}: {best[0]:.3g} bars on {best[1]}")
    assert best[0] >= SEEN, f"no fixture sees '{fault}': at most {best[0]:.3g} bars ({best[1]})"


@pytest.mark.parametrize("fault", ["clip_ignored", "clip_ignored_low", "clip_ignored_high"])
def test_a_clip_that_lets_a_side_through_breaks_the_exact_zeros_of_a_pure_batch(fault):
    """What passes above 1 - 1e-7 is of the order 1 - q of a row's share: no bar relative to a tensor's largest entry can see it.
    The all-high batch is held to `== 0.0` instead, and there the mutant -- in f32, as a kernel would compute it -- leaves
    numbers; the all-low batch does the same for the lower side."""
    side = "low" if fault == "clip_ignored_low" else "high"
    for shape in HG.CLIP_SHAPES:
        for n in HG.PURE_COUNTS:
            fx = HG.pure(*shape, side, n)
            for dtype in (np.float64, np.float32):
                _l, ref = HG.mutant_loss_and_grads(fx.f, fx.y, fx.weights, None, dtype)
                assert all(np.all(g == 0.0) for g in R.flat(ref))
                _l, grads = HG.mutant_loss_and_grads(fx.f, fx.y, fx.weights, fault, dtype)
                assert all(np.any(g != 0.0) for g in R.flat(grads)), (shape, n, dtype)
            other = "high" if side == "low" else "low"
            if fault != "clip_ignored":      # ... and a one-sided fault leaves the other side's batch exact
                _l, grads = HG.mutant_loss_and_grads(HG.pure(*shape, other, n).f, HG.pure(*shape, other, n).y, fx.weights, fault, np.float32)
                assert all(np.all(g == 0.0) for g in R.flat(grads))


# ---- Adam ---------------------------------------------------------------------------------------------------------------------
def _adam_inputs(shape, batch):
    w0, f, y = HG.adam_fixture(*shape, batch)
    g = [a.astype(np.float32) for a in R.flat(R.loss_and_grads(f, y, w0, np.float32)[2])]
    w = R.flat(w0)
    zero = (0,) if batch == "zero" else ()
    m, v = G.adam_moments([a.shape for a in w], seed=11, zero=zero)
    return w, g, m, v, zero


@pytest.mark.parametrize("fault", G.ADAM_FAULTS)
def test_every_adam_mutant_is_seen_at_100_bars_on_the_head_fixtures(fault):
    """train_gates.adam_step with one fault against itself without, on the head's Adam fixtures, in train_gates.adam_bars."""
    best = (0.0, None)
    for batch in ("zero", "signal"):
        w, g, m, v, _zero = _adam_inputs(HG.ADAM_SHAPES[0], batch)
        for case, hyper in G.ADAM_CASES.items():
            for it in G.ADAM_ITERATIONS:
                w1, m1, v1 = G.adam_step(w, g, m, v, it, hyper)
                w2, m2, v2 = G.adam_step(w, g, m, v, it, hyper, fault)
                for i in range(len(w)):
                    bar_m, bar_v, bar_dw = G.adam_bars(m[i], v[i], g[i], w1[i].astype(np.float64) - w[i], it, hyper)
                    with np.errstate(all="ignore"):
                        rs = {"m": np.abs(m2[i].astype(np.float64) - m1[i]) / np.maximum(bar_m, 1e-300), "v": np.abs(v2[i].astype(np.float64) - v1[i]) / np.maximum(bar_v, 1e-300),
                              "dw": np.abs(w2[i].astype(np.float64) - w1[i]) / max(bar_dw, 1e-300)}
                    for nm, r in rs.items():
                        r = float(np.nanmax(np.where(np.isfinite(r), r, 0.0)))      # (t = 0 gives the mutant NaN: not counted)
                        if r > best[0]:
                            best = (r, f"{batch} {case} iterations={it} tensor {i} {nm}")
    print(f"adam {fault}: {best[0]:.3g} bars on {best[1]}")
    assert best[0] >= SEEN, f"no case sees '{fault}': at most {best[0]:.3g} bars ({best[1]})"


@pytest.mark.parametrize("shape", HG.ADAM_SHAPES, ids=str)
def test_the_bar_on_dw_clears_the_rounding_of_the_head_weights(shape):
    """train_gates' clearance check on the head's Adam fixtures, with the reference's own f32 gradient (the GPU test asserts the
    same with the GPU's before it looks at a result); the all-zero batch gives dW1 a gradient of exactly 0 and nothing else."""
    for batch in ("zero", "signal"):
        w, g, m, v, zero = _adam_inputs(shape, batch)
        assert all(np.any(a) for a in g[1:]) and bool(np.any(g[0])) == (batch == "signal")
        for case, hyper in G.ADAM_CASES.items():
            for it in G.ADAM_ITERATIONS:
                w1, m1, v1 = G.adam_step(w, g, m, v, it, hyper)
                for i in range(4):
                    if i in zero:
                        assert np.array_equal(w1[i], w[i]) and not np.any(m1[i]) and not np.any(v1[i])
                        continue
                    bar_dw = G.adam_bars(m[i], v[i], g[i], w1[i].astype(np.float64) - w[i], it, hyper)[2]
                    assert bar_dw > 0 and G.adam_rounding_clearance(w[i], bar_dw) >= 4.0, (batch, case, it, i)
