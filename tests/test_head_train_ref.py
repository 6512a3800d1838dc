"""tests/head_train_ref.py, the float64 reference of head training, against torch autograd in f64 (<= 1e-10), and its own f32
restatement against the bars the GPU tests use: the GPU kernels are f32 too, so the restatement shows how much of each bar
f32 arithmetic itself takes (asserted: under a quarter)."""
import numpy as np
import pytest
import torch

from oracle.oracle_train import KerasAdam, dropout_scale
from tests import head_train_ref as R

SMALL = [(96, 32, 2, 17), (32, 32, 16, 50), (10560, 256, 11, 93)]


def _torch_grads(f, y, w, s0, s1):
    t = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64)      # noqa: E731
    w1, b1, w2, b2 = (t(a).requires_grad_(True) for a in R.flat(w))
    a = t(f) if s0 is None else t(f) * t(s0)
    h = torch.relu(a @ w1 + b1)
    if s1 is not None:
        h = h * t(s1)
    p = torch.softmax(h @ w2 + b2, dim=1)
    q = torch.clamp(p / p.sum(dim=1, keepdim=True), 1e-7, 1 - 1e-7)
    loss = -(t(y) * torch.log(q)).sum(dim=1).mean()
    loss.backward()
    return float(loss.detach()), [g.grad.numpy() for g in (w1, b1, w2, b2)]


@pytest.mark.parametrize("shape", SMALL, ids=str)
@pytest.mark.parametrize("drop", [False, True], ids=["plain", "dropout"])
def test_reference_against_torch_autograd_f64(shape, drop):
    fx = R.fixture(*shape)
    sel = fx.keep_drop if drop else fx.keep
    dropout = dict(fx.dropout, frames=sel) if drop else None
    loss, _li, grads, _p = R.loss_and_grads(fx.f[sel], fx.y[sel], fx.w, np.float64, dropout)
    s0, s1 = R.scales(dropout, len(sel), fx.K, fx.H, np.float64)
    tl, tg = _torch_grads(fx.f[sel], fx.y[sel], fx.w, s0, s1)
    assert abs(loss - tl) <= 1e-10 * abs(tl)
    for g, r in zip(R.flat(grads), tg):
        assert np.abs(r).max() > 0 and R.rel(g, r) <= 1e-10


@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
@pytest.mark.parametrize("drop", [False, True], ids=["plain", "dropout"])
def test_f32_restatement_stays_under_a_quarter_of_the_gradient_bar(shape, drop):
    fx = R.fixture(*shape)
    sel = fx.keep_drop if drop else fx.keep
    dropout = dict(fx.dropout, frames=sel) if drop else None
    loss, _li, grads, _p = R.loss_and_grads(fx.f[sel], fx.y[sel], fx.w, np.float64, dropout)
    l32, _li, g32, _p = R.loss_and_grads(fx.f[sel], fx.y[sel], fx.w, np.float32, dropout)
    errs = [R.rel(a, b) for a, b in zip(R.flat(g32), R.flat(grads))]
    print(shape, drop, "f32 restatement: loss", abs(l32 - loss), "tensors", errs)
    assert abs(l32 - loss) <= 2.5e-6 and max(errs) <= 2.5e-6


def test_dropout_masks_are_the_stated_generator_and_act():
    fx = R.fixture(96, 32, 2, 17)
    s0 = dropout_scale(0.5, fx.dropout["seed"], 0, fx.keep_drop, fx.K, 0)
    assert set(np.unique(s0)) == {0.0, 2.0} and 0.35 < (s0 > 0).mean() < 0.65
    plain = R.loss_and_grads(fx.f[fx.keep_drop], fx.y[fx.keep_drop], fx.w)[2]
    drop = R.loss_and_grads(fx.f[fx.keep_drop], fx.y[fx.keep_drop], fx.w, dropout=dict(fx.dropout, frames=fx.keep_drop))[2]
    assert R.rel(drop[0][0], plain[0][0]) > 0.1


def test_guard_drops_about_one_row_in_a_hundred():
    fx = R.fixture(10560, 256, 11, 257)
    dropped = fx.pool - int(R.guarded(R.forward(fx.f, fx.w)["z1"]).sum())
    print("guard dropped", dropped, "of", fx.pool)
    assert dropped <= R.MAX_DROPPED * fx.pool


@pytest.mark.parametrize("drop", [False, True], ids=["plain", "dropout"])
def test_f32_restatement_of_the_adam_trajectory(drop):
    case = R.adam_case(drop)
    w = [(k.copy(), b.copy()) for k, b in case["w0"]]
    opt = KerasAdam([t.shape for t in R.flat(w)])
    for i in range(case["steps"]):
        idx = case["order"][i * case["batch"]:(i + 1) * case["batch"]]
        R.train_step(case["f"][idx], case["y"][idx], w, opt, np.float32, None if not drop else dict(case["dropout"], frames=idx))
    errs = [float(np.abs(a.astype(np.float64) - b).max()) / m for a, b, m in zip(R.flat(w), R.flat(case["ref"]), case["moved"])]
    print("adam f32 restatement / max|w - w0|:", errs, "losses", case["losses"][0], case["losses"][-1])
    assert case["losses"][-1] < case["losses"][0] or drop
    assert max(errs) <= 2.5e-5


def test_evaluate_counts_hits_with_the_lowest_index_on_a_tie():
    w = [(np.zeros((32, 32), np.float32), np.zeros(32, np.float32)), (np.zeros((32, 3), np.float32), np.zeros(3, np.float32))]
    y = np.array([[1, 0, 0], [0, 1, 0], [0.5, 0.5, 0]], np.float32)      # p is uniform: arg-max 0; rows 0 and 2 hit
    ls, hits = R.evaluate(np.zeros((3, 32), np.float32), y, w)
    assert hits == 2 and abs(ls - (2 * np.log(3) + np.log(3))) < 1e-12
