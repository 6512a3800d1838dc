"""The one fit loop of training.py (_TrainerCore.fit), driven without a GPU: Trainer and HeadTrainer with the five methods that
touch the device replaced by a few lines of numpy -- the "weights" are the number of batches applied so far, the val_loss of
each epoch is scripted -- and the three converters that place data on the device handing numpy through.  Everything else is
the product's: the class attributes of the two trainers, the callback parsing, the epoch loop, early stopping, restore-best."""
import numpy as np
import pytest

from modulationdetectioncnn_amd import training
from modulationdetectioncnn_amd.callbacks import EarlyStopping, ModelCheckpoint

N, BATCH = 10, 4
RANGES = [(0, 4), (4, 4), (8, 2)]                            # an epoch of N samples in batches of BATCH: the last one short
VAL = [5.0, 4.0, 4.5, 3.0, 3.0, 3.5, 1.0, 0.5]               # strictly better at epochs 0, 1, 3; patience 2 runs out at epoch 5


class _Fake:
    def __init__(self, val=VAL, max_batch=None):
        self.calls, self.saved, self.weights, self.val = [], [], 0, list(val)
        self.stats = dict(train=0, evaluated=0)
        if max_batch is not None:
            self.max_batch = self._max_rows = max_batch

    # the converters
    def _samples(self, X):
        return np.asarray(X, np.float32)

    def _targets(self, Y, n):
        assert len(Y) == n
        return np.asarray(Y)

    def _indices(self, order_h):
        assert order_h.dtype == np.int32
        return order_h

    # the device
    def train_batch(self, x, y, order=None, first=0, count=None, apply=True):
        assert apply and sorted(order) == list(range(len(x)))
        self.calls.append(("train", first, count))
        self.weights += 1
        self.stats["train"] += count

    def evaluate_enqueue(self, x, y, order=None, first=0, count=None):
        self.calls.append(("eval", len(x)))
        self.stats["evaluated"] += len(x)

    def read(self, reset=True):
        self.calls.append(("read",))
        nt, ne = self.stats["train"], self.stats["evaluated"]
        val = self.val.pop(0) if ne else 0.0
        r = {"train_loss_sum": 2.0 * nt, f"train_{self._UNIT}s": nt, "eval_loss_sum": val * ne, f"eval_{self._UNIT}s": ne, "iterations": self.weights}
        r.update({field: ne // 2 for field in self._EXTRA.values()})          # half of the validation set is classified right
        if reset:
            self.stats = dict(train=0, evaluated=0)
        return r

    def get_weights(self):
        return self.weights

    def set_weights(self, weights):
        self.calls.append(("set", weights))
        self.weights = weights


class FakeTrainer(_Fake, training.Trainer):
    def save(self, filepath):                                # Trainer.save writes an .h5 from device state
        self.saved.append((filepath, self.weights))


class FakeHead(_Fake, training.HeadTrainer):
    pass


X, Y = np.zeros((N, 3), np.float32), np.zeros(N, np.int64)
VALSET = (np.zeros((6, 3), np.float32), np.zeros(6, np.int64))
BOTH = pytest.mark.parametrize("make", [FakeTrainer, lambda **kw: FakeHead(max_batch=8, **kw)], ids=["trainer", "head"])


def _epochs(calls):
    """The calls between two reads, the initial reset dropped."""
    out, cur = [], []
    for c in calls:
        if c == ("read",):
            out.append(cur)
            cur = []
        else:
            cur.append(c)
    assert cur == [] and out[0] == []
    return out[1:]


@BOTH
def test_an_epoch_is_its_batches_then_the_evaluation_then_one_read(make):
    tr = make()
    hist = tr.fit(X, Y, batch_size=BATCH, epochs=3, validation_data=VALSET, patience=None, seed=1)
    assert _epochs(tr.calls) == [[("train", f, c) for f, c in RANGES] + [("eval", 6)]] * 3
    assert hist.epoch == [0, 1, 2] and hist.history["loss"] == [2.0] * 3 and hist.history["val_loss"] == VAL[:3]
    assert hist.stopped_epoch is None and hist.best_epoch == 1 and hist.best_weights == 6


@BOTH
def test_without_validation_data_nothing_is_evaluated_and_val_loss_is_absent(make):
    tr = make()
    hist = tr.fit(X, Y, batch_size=BATCH, epochs=2, checkpoint="ckpt.h5", save=lambda path: tr.saved.append(path))
    assert _epochs(tr.calls) == [[("train", f, c) for f, c in RANGES]] * 2
    assert sorted(hist.history) == ["loss"] and hist.best_epoch is None and tr.saved == []      # val_loss watched nothing: all epochs, no save


@BOTH
@pytest.mark.parametrize("perm", [list(range(N - 1)), list(range(N - 1)) + [N], [-1] + list(range(1, N))], ids=["short", "too-large", "negative"])
def test_a_bad_permutation_is_refused_before_anything_is_enqueued(make, perm):
    tr = make()
    with pytest.raises(ValueError, match="permutation"):
        tr.fit(X, Y, batch_size=BATCH, epochs=2, permutations=lambda ep: perm)
    assert tr.calls == [("read",)]
    tr = make()
    tr.fit(X, Y, batch_size=BATCH, epochs=1, permutations=lambda ep: list(range(N))[::-1])
    assert len(_epochs(tr.calls)) == 1


@BOTH
def test_patience_stops_at_the_scripted_epoch_and_checkpoints_only_strict_improvements(make):
    tr = make()
    save = {} if isinstance(tr, FakeTrainer) else {"save": lambda path: tr.saved.append((path, tr.weights))}
    hist = tr.fit(X, Y, batch_size=BATCH, epochs=8, validation_data=VALSET, patience=2, checkpoint="best.h5", **save)
    assert hist.stopped_epoch == 5 and hist.epoch == list(range(6)) and hist.best_epoch == 3
    assert hist.history["val_loss"] == VAL[:6] and len(_epochs(tr.calls)) == 6
    assert tr.saved == [("best.h5", 3 * (ep + 1)) for ep in (0, 1, 3)]                          # 3.0 after 3.0 is no improvement
    assert hist.best_weights == 12 and tr.weights == 18                                          # nothing restored unless asked for


@BOTH
def test_restore_best_weights_puts_the_best_epochs_weights_back(make):
    tr = make()
    stop = EarlyStopping(patience=2, restore_best_weights=True)
    hist = tr.fit(X, Y, batch_size=BATCH, epochs=8, validation_data=VALSET, callbacks=[stop])
    assert hist.stopped_epoch == stop.stopped_epoch == 5
    assert tr.calls[-1] == ("set", 12) and tr.weights == 12


@BOTH
def test_callbacks_and_their_short_forms_do_not_mix(make):
    tr = make()
    with pytest.raises(ValueError, match="not both"):
        tr.fit(X, Y, batch_size=BATCH, callbacks=[ModelCheckpoint("a.h5")], checkpoint="b.h5", save=print)
    with pytest.raises(ValueError, match="at most one"):
        tr.fit(X, Y, batch_size=BATCH, callbacks=[EarlyStopping(), EarlyStopping()])
    with pytest.raises(ValueError, match="batch_size"):
        tr.fit(X, Y, batch_size=0)
    assert tr.calls == []


def test_the_head_adds_val_accuracy_and_needs_save_for_a_checkpoint_and_bounds_the_batch():
    tr = FakeHead(max_batch=8)
    hist = tr.fit(X, Y, batch_size=BATCH, epochs=2, validation_data=VALSET, patience=None)
    assert hist.history["val_accuracy"] == [0.5, 0.5] and sorted(hist.history) == ["loss", "val_accuracy", "val_loss"]
    assert sorted(FakeHead(max_batch=8).fit(X, Y, batch_size=BATCH, epochs=1).history) == ["loss"]
    assert "val_accuracy" not in FakeTrainer().fit(X, Y, batch_size=BATCH, epochs=1, validation_data=VALSET).history
    tr = FakeHead(max_batch=8)
    with pytest.raises(ValueError, match="save="):
        tr.fit(X, Y, batch_size=BATCH, validation_data=VALSET, checkpoint="best.h5")
    with pytest.raises(ValueError, match="save="):
        tr.fit(X, Y, batch_size=BATCH, validation_data=VALSET, callbacks=[ModelCheckpoint("best.h5", save_best_only=True)])
    with pytest.raises(ValueError, match="max_batch = 8"):
        tr.fit(X, Y, batch_size=9)
    assert tr.calls == []
    FakeTrainer().fit(X, Y, batch_size=9, epochs=1)                                             # no such bound of the full trainer's own
