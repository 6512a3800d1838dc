"""Head training on the MI355X (csrc/head_train.hip via mdc_head_trainer_* / training.HeadTrainer / VTCNN2.fit_head) against
tests/head_train_ref.py, the float64 reference that tests/test_head_train_ref.py holds to torch autograd.

Bars (the project's training bars): every gradient tensor within 1e-5 of its largest entry and the loss within 1e-5 (relative)
of the f64 reference; a 20-step Adam trajectory within 1e-4 of the reference's max|w - w0| per tensor; losses of a fit and of
VTCNN2.evaluate within 2e-5.  The f32 restatement of the reference on the CPU takes 1e-7 .. 8e-7 of the first, <= 1.7e-5 of the
second (tests/test_head_train_ref.py asserts a quarter of each bar).  Fixture rows are selected on the f64 reference alone
(head_train_ref.guarded) so that no ReLU gate can flip under f32 rounding."""
import ctypes as C

import numpy as np
import pytest

from modulationdetectioncnn_amd import VTCNN2, Topology, _cabi, frontend
from modulationdetectioncnn_amd.training import HeadTrainer, to_onehot
from tests import head_train_ref as R

pytestmark = pytest.mark.gpu


def _dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to("cuda:0")


def _step(tr, f, y, order=None, first=0, count=None, apply=False):
    tr.read()
    tr.train_batch(f, y, order, first, count, apply=apply)
    r = tr.read()
    return r["train_loss_sum"] / max(r["train_rows"], 1), tr.gradients()


def _hold(tag, loss, grads, ref_loss, ref_grads):
    errs = [R.rel(g, r) for g, r in zip(R.flat(grads), R.flat(ref_grads))]
    print(tag, "loss", loss, "ref", ref_loss, "rel", abs(loss - ref_loss) / abs(ref_loss), "dW1 db1 dW2 db2", errs)
    assert abs(loss - ref_loss) <= 1e-5 * abs(ref_loss)
    for r in R.flat(ref_grads):
        assert np.abs(r).max() > 0
    assert max(errs) <= 1e-5, errs


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(R.flat(a), R.flat(b)))


# ---- gradients and loss, apply = 0 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
@pytest.mark.parametrize("mode", ["direct", "order", "dropout"])
def test_gradients_and_loss(shape, mode):
    fx = R.fixture(*shape)
    drop = mode == "dropout"
    tr = HeadTrainer(fx.K, fx.H, fx.C, fx.w, device=0, max_batch=fx.count, dropout=fx.dropout["rates"] if drop else (0.0, 0.0),
                     dropout_seed=fx.dropout["seed"])
    if mode == "direct":
        sel = fx.keep
        loss, grads = _step(tr, _dev(fx.f[sel]), _dev(fx.y[sel]))
    else:
        sel = np.random.default_rng(1).permutation(fx.keep_drop if drop else fx.keep)
        order = np.concatenate([np.zeros(5, np.int64), sel]).astype(np.int32)      # positions 0..4 are not the batch's
        loss, grads = _step(tr, _dev(fx.f), _dev(fx.y), _dev(order), 5, fx.count)
    ref_loss, _li, ref_grads, _p = R.loss_and_grads(fx.f[sel], fx.y[sel], fx.w, np.float64, dict(fx.dropout, frames=sel) if drop else None)
    _hold(f"{shape} {mode}:", loss, grads, ref_loss, ref_grads)
    assert _same(tr.get_weights(), fx.w) and tr.read()["iterations"] == 0


@pytest.fixture(scope="module")
def real():
    """A synthetic f32 VT-CNN2, synth_dataset frames at >= 10 dB, and their Flatten rows from the model's own engine."""
    import torch
    m = VTCNN2.synthetic(Topology.vtcnn2(11), seed=2016, device=0)
    recipe = frontend.synth_recipe(snrs_db=(10, 14, 18))
    X, labels, _snr = frontend.synth_dataset(704 + 352, recipe, seed=5, device=0)
    feat = m.head_features(X)
    torch.cuda.synchronize()
    return dict(m=m, X=X, labels=labels.cpu().numpy().astype(np.int64), feat=feat, f=feat.cpu().numpy())


def test_gradients_on_features_of_a_real_model(real):
    m, f = real["m"], real["f"][:140]
    w = m.get_weights()[2:]
    y = to_onehot(real["labels"][:140], 11)
    assert 0.2 < (f == 0).mean() < 0.8                                     # conv2 + ReLU: about half zeros
    ok = np.flatnonzero(R.guarded(R.forward(f, w)["z1"]))
    assert len(f) - len(ok) <= R.MAX_DROPPED * len(f)
    sel = ok[:128]
    tr = HeadTrainer(10560, 256, 11, w, device=0, max_batch=128)
    loss, grads = _step(tr, real["feat"], _dev(to_onehot(real["labels"], 11)), _dev(sel.astype(np.int32)), 0, 128)
    ref_loss, _li, ref_grads, _p = R.loss_and_grads(f[sel], y[sel], w)
    _hold("real features:", loss, grads, ref_loss, ref_grads)


# ---- exact cases ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(96, 32, 2, 17), (10560, 256, 11, 93)], ids=str)
def test_zero_features_give_exactly_zero_dw1(shape):
    fx = R.fixture(*shape)
    tr = HeadTrainer(fx.K, fx.H, fx.C, fx.w, device=0, max_batch=fx.count)
    _loss, g = _step(tr, _dev(np.zeros((fx.count, fx.K), np.float32)), _dev(fx.y[:fx.count]))
    assert np.all(g[0][0] == 0.0) and np.abs(g[0][1]).max() > 0
    f = fx.f[fx.keep].copy()
    cols = [0, 7, fx.K - 1]
    f[:, cols] = 0.0
    _loss, g = _step(tr, _dev(f), _dev(fx.y[fx.keep]))
    assert np.all(g[0][0][cols] == 0.0) and np.abs(np.delete(g[0][0], cols, axis=0)).max(axis=1).min() > 0


def test_apply_0_changes_nothing_and_a_step_is_bit_identical_from_run_to_run():
    fx = R.fixture(10560, 256, 11, 257)
    f, y = _dev(fx.f[fx.keep]), _dev(fx.y[fx.keep])
    runs = []
    for _ in range(2):
        tr = HeadTrainer(fx.K, fx.H, fx.C, fx.w, device=0, max_batch=fx.count, dropout=(0.5, 0.5), dropout_seed=3)
        l0, g0 = _step(tr, f, y)
        st = tr.optimizer_state()
        assert _same(tr.get_weights(), fx.w) and st["iterations"] == 0
        assert all(not t.any() for t in R.flat(st["m"]) + R.flat(st["v"]))
        l1, g1 = _step(tr, f, y, apply=True)
        assert l1 == l0 and _same(g0, g1) and tr.read()["iterations"] == 1
        assert not _same(tr.get_weights(), fx.w)
        runs.append((l0, g0, tr.get_weights(), tr.optimizer_state()))
    (la, ga, wa, sa), (lb, gb, wb, sb) = runs
    assert la == lb and _same(ga, gb) and _same(wa, wb) and _same(sa["m"], sb["m"]) and _same(sa["v"], sb["v"])


def test_evaluation_ignores_dropout_bit_for_bit():
    fx = R.fixture(10560, 256, 11, 93)
    f, y = _dev(fx.f), _dev(fx.y)
    out = []
    for rates in ((0.0, 0.0), (0.5, 0.5)):
        tr = HeadTrainer(fx.K, fx.H, fx.C, fx.w, device=0, max_batch=64, dropout=rates, dropout_seed=9)      # 93 + rows in calls of 64
        tr.read()
        tr.evaluate_enqueue(f, y)
        out.append(tr.read())
    assert out[0] == out[1] and out[0]["eval_rows"] == fx.pool


# ---- Adam ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("drop", [False, True], ids=["plain", "dropout"])
def test_adam_trajectory_of_20_steps(drop):
    case = R.adam_case(drop)
    d = case["dropout"]
    tr = HeadTrainer(10560, 256, 11, case["w0"], device=0, max_batch=case["batch"], dropout=d["rates"] if drop else (0.0, 0.0),
                     dropout_seed=d["seed"] if drop else 0)
    f, y, order = _dev(case["f"]), _dev(case["y"]), _dev(case["order"])
    for i in range(case["steps"]):
        tr.train_batch(f, y, order, i * case["batch"], case["batch"])
    r = tr.read()
    errs = [float(np.abs(a.astype(np.float64) - b).max()) / mv for a, b, mv in zip(R.flat(tr.get_weights()), R.flat(case["ref"]), case["moved"])]
    ref_sum = float(np.sum(case["losses"])) * case["batch"]
    print("adam", drop, "error / max|w - w0| per tensor", errs, "loss sum", r["train_loss_sum"], "ref", ref_sum)
    assert r["iterations"] == case["steps"] and r["train_rows"] == case["steps"] * case["batch"]
    assert max(errs) <= 1e-4, errs
    assert abs(r["train_loss_sum"] - ref_sum) <= 2e-5 * ref_sum


def test_graph_replay_equals_eager_steps_with_a_new_mask_each_step():
    import torch
    fx = R.fixture(10560, 256, 11, 93)
    f, y = _dev(fx.f[fx.keep]), _dev(fx.y[fx.keep])
    eager, graph = (HeadTrainer(fx.K, fx.H, fx.C, fx.w, device=0, max_batch=fx.count, dropout=(0.5, 0.5), dropout_seed=4) for _ in range(2))
    grads = []
    for _ in range(5):
        eager.train_batch(f, y)
        grads.append(eager.gradients()[0][0])
    assert not np.array_equal(grads[0], grads[1])                          # another step, another mask
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        graph.read()                                                       # (touch the trainer outside the capture)
        with torch.cuda.graph(g, stream=side):
            graph.train_batch(f, y)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(5):
        g.replay()
    torch.cuda.synchronize()
    ra, rb = eager.read(), graph.read()
    assert ra["iterations"] == rb["iterations"] == 5 and ra["train_loss_sum"] == rb["train_loss_sum"]
    assert _same(eager.get_weights(), graph.get_weights()) and _same(eager.gradients(), graph.gradients())


# ---- statistics and refusals ------------------------------------------------------------------------------------------------------
def test_evaluation_statistics_against_the_reference():
    fx = R.fixture(32, 32, 16, 50)
    tr = HeadTrainer(fx.K, fx.H, fx.C, fx.w, device=0, max_batch=fx.pool)
    y = fx.y.copy()
    y[1] = 0.0
    y[1, [3, 9]] = 0.5                                                     # a tie in the target row: its lowest index counts
    tr.read()
    tr.evaluate_enqueue(_dev(fx.f), _dev(y))
    r = tr.read()
    ls, hits = R.evaluate(fx.f, y, fx.w)
    print("eval", r, "ref", ls, hits)
    assert r["eval_rows"] == fx.pool and r["eval_correct"] == hits and abs(r["eval_loss_sum"] - ls) <= 1e-5 * ls
    assert r["train_rows"] == 0 and tr.read()["eval_rows"] == 0             # the read reset them


def test_evaluation_agrees_with_the_model_it_came_from(real):
    m = real["m"]
    X, lab = real["X"][704:], real["labels"][704:]
    tr = HeadTrainer(10560, 256, 11, m.get_weights()[2:], device=0, max_batch=512)
    loss, acc = tr.evaluate(real["feat"][704:], lab)
    ref_loss, ref_hits = R.evaluate(real["f"][704:], to_onehot(lab, 11), m.get_weights()[2:])
    model_loss = m.evaluate(X, lab)
    print("evaluate: head", loss, "model", model_loss, "f64 reference", ref_loss / len(lab), "accuracy", acc, ref_hits / len(lab))
    assert abs(loss - ref_loss / len(lab)) <= 1e-5 * loss and acc == ref_hits / len(lab)
    assert abs(loss - model_loss) <= 2e-5 * loss
    assert acc == float((m.predict_classes(X).cpu().numpy() == lab).mean())


def test_an_index_out_of_range_is_skipped_counted_and_reported_at_the_read():
    fx = R.fixture(96, 32, 2, 17)
    tr = HeadTrainer(fx.K, fx.H, fx.C, fx.w, device=0, max_batch=32)
    sel = fx.keep
    order = np.concatenate([sel[:9], [fx.pool, -1], sel[9:]]).astype(np.int32)
    tr.read()
    tr.train_batch(_dev(fx.f), _dev(fx.y), _dev(order), 0, len(order), apply=False)
    with pytest.raises(_cabi.MdcError, match="2 batch positions") as e:
        tr.read()
    assert e.value.code == -22
    ref_loss, _li, ref_grads, _p = R.loss_and_grads(fx.f[sel], fx.y[sel], fx.w, divide_by=len(order))
    assert max(R.rel(g, r) for g, r in zip(R.flat(tr.gradients()), R.flat(ref_grads))) <= 1e-5
    r = tr.read()                                                          # the count was reset with the statistics
    assert r["train_rows"] == 0


def test_refusals():
    import torch
    L = _cabi.lib()
    h = C.c_void_p()
    for K, H, Cn, mb, word in ((48, 32, 2, 8, b"features"), (96, 40, 2, 8, b"hidden"), (96, 32, 1, 8, b"classes"), (96, 32, 17, 8, b"classes"),
                               (96, 32, 2, 0, b"max_batch"), (96, 32, 2, 65537, b"max_batch"), (16416, 32, 2, 8, b"features"), (96, 288, 2, 8, b"hidden")):
        assert L.mdc_head_trainer_create(K, H, Cn, mb, 0, C.byref(h)) == -22 and word in L.mdc_last_error(), (K, H, Cn, mb)
        assert not h.value
    fx = R.fixture(96, 32, 2, 17)
    f, y = _dev(fx.f), _dev(fx.y)
    tr = HeadTrainer(fx.K, fx.H, fx.C, None, device=0, max_batch=8)
    with pytest.raises(_cabi.MdcError, match="no weights") as e:           # a batch before the weights are set: a state error
        tr.train_batch(f, y, None, 0, 8)
    assert e.value.code != -22
    tr._set(_cabi.TRAIN_WEIGHTS, fx.w)
    tr.train_batch(f, y, None, 0, 8)
    with pytest.raises(_cabi.MdcError, match="max_batch") as e:
        tr.train_batch(f, y, None, 0, 9)
    assert e.value.code == -22
    assert L.mdc_head_trainer_evaluate(tr._h, f.data_ptr(), y.data_ptr(), fx.pool, None, 0, 9, None) == -22 and b"max_batch" in L.mdc_last_error()
    with pytest.raises(ValueError, match="16-byte"):                        # rows that start 4 bytes into an allocation
        tr.train_batch(torch.zeros(fx.pool * fx.K + 1, device="cuda:0")[1:].view(fx.pool, fx.K), y, None, 0, 8)
    assert L.mdc_head_train_batch(tr._h, f.data_ptr() + 4, y.data_ptr(), fx.pool - 1, None, 0, 8, 0, None) == -22 and b"aligned" in L.mdc_last_error()
    for bad in (torch.from_numpy(fx.f), f.double(), f[:, :64]):             # a host tensor, another dtype, another width
        with pytest.raises(ValueError):
            tr.train_batch(bad, y, None, 0, 8)
    with pytest.raises(ValueError):
        tr.train_batch(f, y.cpu(), None, 0, 8)
    with pytest.raises(ValueError):
        tr.train_batch(f, y, torch.zeros(8, dtype=torch.int64, device="cuda:0"), 0, 8)
    with pytest.raises(ValueError):
        HeadTrainer(fx.K, fx.H, fx.C, [fx.w[1], fx.w[0]], device=0, max_batch=8)
    with pytest.raises(_cabi.MdcError):
        HeadTrainer(fx.K, fx.H, fx.C, fx.w, device=0, max_batch=8, dropout=(1.0, 0.0))
    with pytest.raises(ValueError, match="vtcnn2"):
        VTCNN2.synthetic("deployed3", device=0).fit_head(np.zeros((4, 2, 128), np.float32), np.zeros(4, np.int64))
    with pytest.raises(ValueError, match=r"337920 bytes.* 1000"):           # 8 frames x 10560 x 4 bytes against a budget of 1000
        VTCNN2.synthetic("vtcnn2", device=0).fit_head(np.zeros((8, 2, 128), np.float32), np.zeros(8, np.int64), feature_budget_bytes=1000)


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def test_fit_head_end_to_end(real, tmp_path):
    from modulationdetectioncnn_amd.formats.h5mini import H5File
    m = VTCNN2.synthetic(Topology.vtcnn2(11), seed=2016, device=0)
    w0 = m.get_weights()
    X, lab = real["X"], real["labels"]
    Xt, Xv, yt, yv = X[:704], X[704:], to_onehot(lab[:704], 11), to_onehot(lab[704:], 11)
    perms = [np.random.default_rng(40 + ep).permutation(704) for ep in range(3)]
    ckpt = str(tmp_path / "head.h5")
    hist = m.fit_head(Xt, yt, batch_size=64, epochs=3, validation_data=(Xv, yv), dropout=(0.0, 0.0), permutations=lambda ep: perms[ep],
                      patience=None, checkpoint=ckpt)
    ref = R.fit(w0[2:], real["f"][:704], yt, 64, 3, (real["f"][704:], yv), lambda ep: perms[ep])
    print("fit_head loss", hist.history["loss"], "ref", ref["loss"], "val_loss", hist.history["val_loss"], "ref", ref["val_loss"],
          "val_accuracy", hist.history["val_accuracy"], "ref", ref["val_accuracy"])
    for key in ("loss", "val_loss"):
        assert len(hist.history[key]) == 3
        for a, b in zip(hist.history[key], ref[key]):
            assert abs(a - b) <= 2e-5 * b, (key, a, b)
    assert hist.history["loss"][-1] < hist.history["loss"][0]
    assert m.head_history is hist and hist.epoch == [0, 1, 2]
    # predict afterwards uses the new head, the conv layers are the old ones bit for bit
    assert abs(m.evaluate(Xv, yv) - hist.history["val_loss"][-1]) <= 2e-5 * hist.history["val_loss"][-1]
    w1 = m.get_weights()
    assert _same(w1[:2], w0[:2]) and not _same(w1[2:], w0[2:])
    # the checkpoint: the whole model at the best epoch, no optimiser state
    best = VTCNN2.from_h5(ckpt, device=0)
    assert _same(best.get_weights()[:2], w0[:2]) and _same(best.get_weights()[2:], hist.best_weights)
    assert "optimizer_weights" not in H5File(ckpt).root.children
    # another class list: a fresh dense2, the fitted dense1, a new model; the old one is left alone
    lab12 = lab[:704].copy()
    lab12[::7] = 11
    # epochs = 0: nothing is trained, so what the new model holds is what fit_head handed the trainer -- the FITTED dense1, bit for bit
    # (a re-initialised dense1 would differ), a fresh seeded dense2, the old conv layers; the old model keeps its eleven classes
    m12 = m.fit_head(Xt, lab12, batch_size=64, epochs=0, classes=12, seed=3, patience=None)
    assert isinstance(m12, VTCNN2) and m12.topology == Topology.vtcnn2(12) and _same(m.get_weights(), w1)
    assert m.topology == Topology.vtcnn2(11) and m.get_weights()[3][0].shape == (256, 11)
    w12 = m12.get_weights()
    assert _same(w12[:3], w1[:3]) and w12[3][0].shape == (256, 12) and np.abs(w12[3][0]).max() > 0 and not w12[3][1].any()
    again = m.fit_head(Xt, lab12, batch_size=64, epochs=0, classes=12, seed=3, patience=None).get_weights()
    other = m.fit_head(Xt, lab12, batch_size=64, epochs=0, classes=12, seed=4, patience=None).get_weights()
    assert np.array_equal(again[3][0], w12[3][0]) and not np.array_equal(other[3][0], w12[3][0])      # Glorot, seeded
    # ... and one epoch from there moves both dense layers of the new model only
    m12 = m.fit_head(Xt, lab12, batch_size=64, epochs=1, dropout=(0.5, 0.5), classes=12, seed=3, patience=None)
    v12 = m12.get_weights()
    assert _same(v12[:2], w0[:2]) and not np.array_equal(v12[2][0], w1[2][0]) and not np.array_equal(v12[3][0], w12[3][0])
    assert np.abs(v12[2][0] - w1[2][0]).max() < 0.05 and _same(m.get_weights(), w1)                   # fine-tuned from the fitted one
    assert m12.predict(Xv).shape == (352, 12) and len(m12.head_history.history["loss"]) == 1


# ---- count below max_batch: the scratch is sized for max_batch, the plan (K-slices, batch slices) follows count ----------------------
# (max_batch, count): at VT-CNN2's shape launch 3 takes min(3, stages of 32 rows) slices of whole stages -- 96 rows are three one-stage
# slices, 128 rows two two-stage ones, so the number of partial dW1 tensors is not monotone in count; 1 row and a full batch beside them
@pytest.mark.parametrize("max_batch,count", [(128, 96), (128, 65), (128, 128), (160, 97), (257, 225), (257, 1), (1024, 96)], ids=str)
def test_count_below_max_batch(max_batch, count):
    fx = R.fixture(10560, 256, 11, 257)
    sel = fx.keep[:count]
    tr = HeadTrainer(fx.K, fx.H, fx.C, fx.w, device=0, max_batch=max_batch)
    loss, grads = _step(tr, _dev(fx.f), _dev(fx.y), _dev(sel.astype(np.int32)), 0, count)
    ref_loss, _li, ref_grads, _p = R.loss_and_grads(fx.f[sel], fx.y[sel], fx.w)
    _hold(f"max_batch {max_batch} count {count}:", loss, grads, ref_loss, ref_grads)
    # one applied step at this count, then a full batch on the same trainer: both against the reference's two steps
    w = [(k.copy(), b.copy()) for k, b in fx.w]
    opt = R.KerasAdam([t.shape for t in R.flat(w)])
    full = fx.keep[:min(max_batch, 257)]
    R.train_step(fx.f[sel], fx.y[sel], w, opt)
    R.train_step(fx.f[full], fx.y[full], w, opt)
    tr.train_batch(_dev(fx.f), _dev(fx.y), _dev(sel.astype(np.int32)), 0, count)
    tr.train_batch(_dev(fx.f), _dev(fx.y), _dev(full.astype(np.int32)), 0, len(full))
    assert tr.read()["iterations"] == 2
    errs = [float(np.abs(a.astype(np.float64) - b).max()) / max(float(np.abs(b.astype(np.float64) - c).max()), 1e-30)
            for a, b, c in zip(R.flat(tr.get_weights()), R.flat(w), R.flat(fx.w))]
    print("two steps, error / max|w - w0| per tensor", errs)
    assert max(errs) <= 1e-4, errs


def test_fit_with_a_short_last_batch():
    """200 rows at batch 128: every epoch ends in a batch of 72 rows (three batch slices in launch 3 where the full batch has two)."""
    fx = R.fixture(10560, 256, 11, 257)
    f, y, fv, yv = fx.f[:200], fx.y[:200], fx.f[200:], fx.y[200:]
    perms = [np.random.default_rng(60 + ep).permutation(200) for ep in range(2)]
    tr = HeadTrainer(fx.K, fx.H, fx.C, fx.w, device=0, max_batch=128)
    hist = tr.fit(f, y, batch_size=128, epochs=2, validation_data=(fv, yv), permutations=lambda ep: perms[ep], patience=None)
    ref = R.fit(fx.w, f, y, 128, 2, (fv, yv), lambda ep: perms[ep])
    print("short last batch: loss", hist.history["loss"], ref["loss"], "val_loss", hist.history["val_loss"], ref["val_loss"])
    for key in ("loss", "val_loss"):
        for a, b in zip(hist.history[key], ref[key]):
            assert abs(a - b) <= 2e-5 * b, (key, a, b)
    assert hist.history["val_accuracy"] == ref["val_accuracy"] and tr.read()["iterations"] == 4
    moved = [float(np.abs(b.astype(np.float64) - c).max()) for b, c in zip(R.flat(ref["weights"]), R.flat(fx.w))]
    errs = [float(np.abs(a.astype(np.float64) - b).max()) / mv for a, b, mv in zip(R.flat(tr.get_weights()), R.flat(ref["weights"]), moved)]
    assert max(errs) <= 1e-4, errs
