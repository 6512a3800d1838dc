"""Host-side mirror of the reference's training calls, over libmdc.so's mdc_trainer_* entry points.

    reference (cnn.py / CNN.ipynb)                                        here
    -------------------------------------------------------------------   ------------------------------------------
    model.compile(loss='categorical_crossentropy', optimizer='adam')      Trainer(topology, weights)        cnn.py:113
    history = model.fit(X_train, Y_train, batch_size=1024, epochs=100,    history = m.fit(X_train, Y_train, batch_size=1024,
        validation_data=(X_test, Y_test), callbacks=[                         epochs=100, validation_data=(X_test, Y_test),
        ModelCheckpoint(filepath, monitor='val_loss', save_best_only=True),   checkpoint=filepath,
        EarlyStopping(monitor='val_loss', patience=5)])                       patience=5)                   cnn.py:135-146
    model.load_weights(filepath)                                          m.load_weights(filepath)          cnn.py:147
    history.epoch, history.history['loss'], ['val_loss']                  the same attributes               cnn.py:164-166

Scope: the two nets the reference trains -- Topology.deployed (CNN.ipynb cell 6) and Topology.cnnpy (cnn.py:104-112) --
in f32.  All arithmetic (forward, loss, backward, Adam) runs in hand-written gfx950 kernels (csrc/train.hip); there is no
CPU fallback.  The training set is placed in HBM once; an epoch's shuffle is an index array, a mini-batch two launches,
and the host reads one pair of numbers (loss, val_loss) per epoch.

The canonical VT-CNN2 is not trained end to end; HeadTrainer (mdc_head_trainer_*, csrc/head_train.hip) trains its dense layers --
95 % of its parameters -- on precomputed feature rows with the conv layers frozen, and VTCNN2.fit_head drives it.  The two
trainers differ in their kernels, not in their bookkeeping: both are a _TrainerCore, which owns the handle, the parameter
vectors, the steps, the statistics and the one fit loop; a subclass states its entry points, its words and its shapes.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _cabi
from .topology import Topology

_KIND = {"deployed": _cabi.KIND_DEPLOYED, "vtcnn2": _cabi.KIND_VTCNN2, "cnnpy": _cabi.KIND_CNNPY}
ADAM_DEFAULTS = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-7)      # keras.optimizers.Adam(); every bundled .h5's training_config

Weights = List[Tuple[np.ndarray, np.ndarray]]


def _torch():
    import torch
    return torch


def to_onehot(labels, classes: Optional[int] = None) -> np.ndarray:
    """cnn.py:74-81 (`yy1[np.arange(len(data)), data] = 1`), float32."""
    lab = np.asarray(labels).astype(np.int64).reshape(-1)
    classes = int(lab.max()) + 1 if classes is None else int(classes)
    if lab.size and (lab.min() < 0 or lab.max() >= classes):
        raise ValueError(f"labels lie outside [0, {classes})")
    out = np.zeros((lab.size, classes), np.float32)
    out[np.arange(lab.size), lab] = 1.0
    return out


class History:
    """What Keras' fit returns, as far as the reference reads it (cnn.py:164-166): .epoch and .history[...]."""

    def __init__(self):
        self.epoch: List[int] = []
        self.history: Dict[str, List[float]] = {"loss": [], "val_loss": []}
        self.best_epoch: Optional[int] = None
        self.stopped_epoch: Optional[int] = None      # EarlyStopping.stopped_epoch (None: ran all epochs)
        self.best_weights: Optional[Weights] = None

    def __repr__(self):
        return f"History(epochs={len(self.epoch)}, best_epoch={self.best_epoch}, stopped_epoch={self.stopped_epoch})"


class _TrainerCore:
    """What Trainer and HeadTrainer share -- everything but the kernels behind them: the handle, the four parameter vectors, the
    device-resident data set, the steps, the statistics and the fit loop (the host half in C is csrc/train_host.hip).  A subclass
    states what differs in the class attributes below, sets `layer_shapes`, `classes` and `_tail` and creates its handle."""

    _PREFIX = ""             # entry points: _PREFIX + "set_tensor", ...; the one irregular name is _TRAIN_BATCH
    _TRAIN_BATCH = ""
    _UNIT = ""               # what one sample is: read()'s train_<unit>s / eval_<unit>s, and the word in messages
    _SAMPLES = ""            # what the samples are called
    _ALIGN16 = False         # the sample pointer must be 16-byte aligned
    _EXTRA = {}              # epoch metric -> the read() field it is the per-sample mean of, behind val_loss
    save = None              # save(filepath) writes a checkpoint; a trainer without one needs fit(save=)

    layer_shapes: Sequence = ()      # ((kernel shape, bias shape), ...) in Keras' layouts
    classes = 0
    _tail: Tuple[int, ...] = ()      # shape of one sample
    _max_rows: Optional[int] = None  # samples one train_batch / evaluate call may take (None: no limit of the trainer's own)
    _h = None

    # ------------------------------------------------------------------ plumbing
    def _open(self, device: Optional[int], variant: str) -> None:
        """Picks the library and the device; the subclass's *_create fills self._h next."""
        torch = _torch()
        if not torch.cuda.is_available():
            raise RuntimeError("no ROCm device visible: the MI355X training path has no CPU fallback")
        self._variant = variant
        self.device_index = torch.cuda.current_device() if device is None else int(device)
        self._h = C.c_void_p()

    def _lib(self):
        return _cabi.lib(self._variant)

    def _fn(self, name: str):
        return getattr(self._lib(), self._PREFIX + name)

    def _check(self, rc: int) -> int:
        return _cabi.check(rc, self._variant)

    def _device(self):
        return _torch().device("cuda", self.device_index)

    def _stream(self):
        return _torch().cuda.current_stream(self._device()).cuda_stream

    def _set_adam(self, lr: float, beta1: float, beta2: float, eps: float) -> None:
        self.adam = dict(lr=float(lr), beta1=float(beta1), beta2=float(beta2), eps=float(eps))
        self._check(self._fn("set_adam")(self._h, *[self.adam[k] for k in ("lr", "beta1", "beta2", "eps")]))

    def close(self) -> None:
        if self._h is not None and self._h.value:
            self._fn("destroy")(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _set(self, which: int, tensors: Sequence[Tuple[np.ndarray, np.ndarray]]) -> None:
        shapes = self.layer_shapes
        if len(tensors) != len(shapes):
            raise ValueError(f"expected {len(shapes)} (kernel, bias) pairs, got {len(tensors)}")
        fp = C.POINTER(C.c_float)
        for i, ((k, b), (ks, bs)) in enumerate(zip(tensors, shapes)):
            k = np.ascontiguousarray(k, dtype=np.float32)
            b = np.ascontiguousarray(b, dtype=np.float32)
            if tuple(k.shape) != ks or tuple(b.shape) != bs:
                raise ValueError(f"layer {i}: expected kernel {ks} bias {bs}, got {k.shape} {b.shape}")
            self._check(self._fn("set_tensor")(self._h, which, i, k.ctypes.data_as(fp), k.size, b.ctypes.data_as(fp), b.size, self._stream()))

    def _get(self, which: int) -> Weights:
        fp = C.POINTER(C.c_float)
        out = []
        for i, (ks, bs) in enumerate(self.layer_shapes):
            k, b = np.empty(ks, np.float32), np.empty(bs, np.float32)
            self._check(self._fn("get_tensor")(self._h, which, i, k.ctypes.data_as(fp), k.size, b.ctypes.data_as(fp), b.size, self._stream()))
            out.append((k, b))
        return out

    # ------------------------------------------------------------------ state
    def get_weights(self) -> Weights:
        return self._get(_cabi.TRAIN_WEIGHTS)

    def set_weights(self, weights) -> None:
        self._set(_cabi.TRAIN_WEIGHTS, weights)

    def gradients(self) -> Weights:
        """d(mean loss)/d(weights) of the last train_batch, in the weights' layouts."""
        return self._get(_cabi.TRAIN_GRADIENT)

    def optimizer_state(self) -> Dict:
        """What the /optimizer_weights group of a Keras full-model .h5 holds: Adam's iter, m and v per tensor."""
        return {"iterations": self.read(reset=False)["iterations"], "m": self._get(_cabi.TRAIN_ADAM_M), "v": self._get(_cabi.TRAIN_ADAM_V)}

    def set_optimizer_state(self, state: Dict) -> None:
        self._set(_cabi.TRAIN_ADAM_M, state["m"])
        self._set(_cabi.TRAIN_ADAM_V, state["v"])
        self._check(self._fn("set_iterations")(self._h, int(state["iterations"]), self._stream()))

    # ------------------------------------------------------------------ data
    def _samples(self, X):
        torch = _torch()
        x = X if isinstance(X, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(X), dtype=np.float32))
        x = x.to(device=self._device(), dtype=torch.float32).contiguous()
        if tuple(x.shape[1:]) != self._tail:
            raise ValueError(f"expected {self._SAMPLES} of shape (n,{','.join(map(str, self._tail))}); got {tuple(x.shape)}")
        return x

    def _targets(self, Y, n: int):
        torch = _torch()
        Cn = self.classes
        y = Y if isinstance(Y, torch.Tensor) else torch.from_numpy(np.asarray(Y))
        if y.ndim == 1:                         # class indices -> the one-hot rows of cnn.py:74-82
            if y.numel() and (int(y.min()) < 0 or int(y.max()) >= Cn):
                raise ValueError(f"labels lie outside [0, {Cn})")
            y = torch.nn.functional.one_hot(y.to(torch.int64), Cn)
        y = y.to(device=self._device(), dtype=torch.float32).contiguous()
        if tuple(y.shape) != (n, Cn):
            raise ValueError(f"expected targets of shape ({n},{Cn}) or ({n},); got {tuple(y.shape)}")
        return y

    def _indices(self, order_h: np.ndarray):
        """An epoch's shuffle (int32, already checked) as the device tensor train_batch takes."""
        return _torch().from_numpy(order_h).to(self._device())

    # ------------------------------------------------------------------ steps
    def _resident(self, x, y, order=None) -> None:
        """The raw pointers below are dereferenced by the kernels: refuse anything that is not a contiguous tensor of the expected
        type in THIS device's memory (a host tensor's data_ptr() would be a GPU fault, not an error).  The VALUES of `order` are
        checked where they are read, on the device: a position that names no sample of x is skipped and the next read() raises
        (fit() also checks the permutations it is given on the host, before anything is enqueued)."""
        torch = _torch()
        want = ((self._SAMPLES, x, torch.float32, self._tail), ("targets", y, torch.float32, (self.classes,)))
        for name, t, dt, tail in want + ((("order", order, torch.int32, ()),) if order is not None else ()):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device.index != self.device_index or t.dtype != dt \
                    or not t.is_contiguous() or tuple(t.shape[1:]) != tail:
                raise ValueError(f"{name}: expected a contiguous {dt} tensor (n,{','.join(map(str, tail))}) on cuda:{self.device_index}")
        if self._ALIGN16 and x.data_ptr() % 16:
            raise ValueError(f"{self._SAMPLES}: the {self._UNIT}s must start at a 16-byte aligned address")
        if y.shape[0] != x.shape[0]:
            raise ValueError(f"{x.shape[0]} {self._UNIT}s but {y.shape[0]} target rows")

    def _range(self, x, order, first: int, count: Optional[int]) -> int:
        n = x.shape[0] if order is None else order.shape[0]
        count = n - first if count is None else int(count)
        if first < 0 or count < 0 or first + count > n:
            raise ValueError(f"batch [{first}, {first + count}) outside the {n} {self._UNIT}s")
        return count

    def train_batch(self, x, y, order=None, first: int = 0, count: Optional[int] = None, apply: bool = True) -> None:
        """model.train_on_batch on samples order[first:first+count] of the device-resident set (x, y); enqueue only.  A trainer
        with a `max_batch` takes at most that many per call."""
        self._resident(x, y, order)
        count = self._range(x, order, first, count)
        self._check(getattr(self._lib(), self._TRAIN_BATCH)(self._h, x.data_ptr(), y.data_ptr(), x.shape[0], order.data_ptr() if order is not None else None,
                                                            first, count, int(apply), self._stream()))

    def evaluate_enqueue(self, x, y, order=None, first: int = 0, count: Optional[int] = None) -> None:
        """Adds the samples' loss sum and their number (and what else the trainer counts) to the evaluation statistics; a trainer
        with a `max_batch` does it in calls of at most that many."""
        self._resident(x, y, order)
        count = self._range(x, order, first, count)
        step = self._max_rows or count          # (no limit: one call, also for no samples at all)
        for s in range(first, first + count, step) if step else (first,):
            self._check(self._fn("evaluate")(self._h, x.data_ptr(), y.data_ptr(), x.shape[0], order.data_ptr() if order is not None else None,
                                             s, min(step, first + count - s), self._stream()))

    def read(self, reset: bool = True) -> Dict:
        """The statistics since the last reset and Adam's step count: the one call here that waits for the device."""
        tl, el = C.c_double(), C.c_double()
        tn, en, it = C.c_int64(), C.c_int64(), C.c_int64()
        extra = {field: C.c_int64() for field in self._EXTRA.values()}
        self._check(self._fn("read")(self._h, int(reset), C.byref(tl), C.byref(tn), C.byref(el), C.byref(en), *map(C.byref, extra.values()),
                                     C.byref(it), self._stream()))
        return {"train_loss_sum": tl.value, f"train_{self._UNIT}s": tn.value, "eval_loss_sum": el.value, f"eval_{self._UNIT}s": en.value,
                **{field: v.value for field, v in extra.items()}, "iterations": it.value}

    def _epoch_logs(self, r: Dict, validated: bool) -> Dict:
        """One read() as Keras' logs: loss, val_loss and the trainer's further validation metrics (None without validation data)."""
        ne = max(r[f"eval_{self._UNIT}s"], 1)
        logs = {"loss": r["train_loss_sum"] / max(r[f"train_{self._UNIT}s"], 1), "val_loss": r["eval_loss_sum"] / ne if validated else None}
        logs.update({metric: r[field] / ne if validated else None for metric, field in self._EXTRA.items()})
        return logs

    def _evaluate(self, X, Y) -> Dict:
        x = self._samples(X)
        y = self._targets(Y, x.shape[0])
        self.read(reset=True)
        self.evaluate_enqueue(x, y)
        return self._epoch_logs(self.read(reset=True), True)

    def loss_and_gradients(self, X, Y) -> Tuple[float, Weights]:
        """Mean loss of one batch and its gradient, nothing applied (the test hook for the backward pass)."""
        x = self._samples(X)
        y = self._targets(Y, x.shape[0])
        self.read(reset=True)
        self.train_batch(x, y, apply=False)
        return self._epoch_logs(self.read(reset=True), False)["loss"], self.gradients()

    # ------------------------------------------------------------------ the loop of cnn.py:135-146
    def fit(self, X, Y, batch_size: int = 1024, epochs: int = 100, validation_data=None, patience: Optional[int] = 5,
            checkpoint: Optional[str] = None, shuffle: bool = True, seed: Optional[int] = None, permutations=None,
            verbose: int = 0, on_best=None, callbacks=None, save=None) -> History:
        """model.fit(X, Y, batch_size, epochs, validation_data=(Xv, Yv), callbacks=[ModelCheckpoint(checkpoint,
        monitor='val_loss', save_best_only=True), EarlyStopping(monitor='val_loss', patience=patience)]) -- pass the two
        callbacks themselves (callbacks.py: cnn.py:143-144 verbatim) or their short forms `checkpoint=` / `patience=`.
        Every epoch trains on a fresh shuffle (numpy Generator(seed); Keras' own shuffle is unseeded) in batches of
        batch_size -- the last one short --, then computes val_loss; an improvement (strictly smaller) saves the
        checkpoint and resets the patience counter, `patience` epochs without one stop the run.  Without
        validation_data a callback that monitors val_loss watches nothing (Keras warns and skips it): all epochs run,
        nothing is saved.  `permutations(epoch)` overrides the shuffle (tests).  on_best(epoch, val_loss, trainer): called
        whenever val_loss improves on every earlier epoch.  The data set is placed on the device once, an epoch's shuffle is
        an index array, and the host reads once per epoch.  A checkpoint is written by save(filepath): the trainer's own, or
        the caller's where the trainer knows only a part of the model (HeadTrainer: VTCNN2.fit_head passes one that writes the
        whole model's .h5)."""
        from .callbacks import EarlyStopping, ModelCheckpoint
        if callbacks is not None:
            if checkpoint is not None:
                raise ValueError("pass callbacks=[ModelCheckpoint(...)] or checkpoint=..., not both")
            ckpts = [c for c in callbacks if isinstance(c, ModelCheckpoint)]
            stops = [c for c in callbacks if isinstance(c, EarlyStopping)]
            if len(ckpts) + len(stops) != len(callbacks) or len(ckpts) > 1 or len(stops) > 1:
                raise ValueError("callbacks: at most one ModelCheckpoint and one EarlyStopping of this package's callbacks module")
            ckpt, stop = (ckpts or [None])[0], (stops or [None])[0]
        else:
            ckpt = ModelCheckpoint(checkpoint, save_best_only=True) if checkpoint is not None else None
            stop = EarlyStopping(patience=int(patience)) if patience is not None else None
        save = save if save is not None else self.save
        if ckpt is not None and save is None:
            raise ValueError("a checkpoint needs save=: a callable (filepath) that writes the model this head belongs to")
        for c in (ckpt, stop):
            if c is not None:
                c.reset()
        x = self._samples(X)
        n = x.shape[0]
        y = self._targets(Y, n)
        if n == 0:
            raise ValueError(f"fit needs at least one {self._UNIT}")
        if batch_size < 1 or (self._max_rows is not None and batch_size > self._max_rows):
            raise ValueError("batch_size must be >= 1" if self._max_rows is None else f"batch_size must lie in 1..max_batch = {self._max_rows}")
        xv = yv = None
        if validation_data is not None:
            xv = self._samples(validation_data[0])
            yv = self._targets(validation_data[1], xv.shape[0])
        rng = np.random.default_rng(seed)
        hist = History()
        hist.history.update({metric: [] for metric in self._EXTRA})
        best, restore = np.inf, None
        self.read(reset=True)
        for ep in range(int(epochs)):
            if permutations is not None:
                order_h = np.asarray(permutations(ep), dtype=np.int32)
            else:
                order_h = (rng.permutation(n) if shuffle else np.arange(n)).astype(np.int32)
            if order_h.shape != (n,) or (n and (int(order_h.min()) < 0 or int(order_h.max()) >= n)):
                raise ValueError(f"a permutation needs one index in [0, {n}) per {self._UNIT}")
            order = self._indices(order_h)
            for s in range(0, n, batch_size):
                self.train_batch(x, y, order, s, min(batch_size, n - s), apply=True)
            if xv is not None:
                self.evaluate_enqueue(xv, yv)
            logs = self._epoch_logs(self.read(reset=True), xv is not None)      # the epoch's one synchronisation
            loss, val = logs["loss"], logs["val_loss"]
            hist.epoch.append(ep)
            for key, value in logs.items():
                if value is not None:
                    hist.history[key].append(value)
            if verbose:
                print(f"Epoch {ep + 1}/{epochs}" + "".join(f" - {key}: {value:.4f}" for key, value in logs.items() if value is not None))
            if val is not None and val < best:
                best, hist.best_epoch = val, ep
                hist.best_weights = self.get_weights()
                if on_best is not None:
                    on_best(ep, val, self)
            if ckpt is not None and ckpt.should_save(logs[ckpt.monitor]):
                save(ckpt.filepath)
            if stop is not None:
                improved, halt = stop.update(logs[stop.monitor])
                if improved and stop.restore_best_weights:
                    restore = self.get_weights()
                if halt:
                    hist.stopped_epoch = stop.stopped_epoch = ep
                    if stop.restore_best_weights and restore is not None:
                        self.set_weights(restore)
                    break
        if xv is None:
            for key in ("val_loss", *self._EXTRA):
                hist.history.pop(key)
        return hist


class Trainer(_TrainerCore):
    """The compiled model's training state on one MI355X: f32 master weights, Adam moments, step count."""

    _PREFIX, _TRAIN_BATCH = "mdc_trainer_", "mdc_train_batch"
    _UNIT, _SAMPLES = "frame", "frames"
    _tail = (2, 128)

    def __init__(self, topology: Topology, weights: Sequence[Tuple[np.ndarray, np.ndarray]], device: Optional[int] = None,
                 lr: float = 1e-3, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-7, dropout: float = 0.0,
                 dropout_seed: int = 0, _lib_variant: str = "product"):
        """dropout: OPTIONAL Dropout(rate) behind the conv activations (and cnn.py's Dense(10)) in training batches -- 0, the
        default, is the reference's nets, which contain no Dropout layer (mdc_trainer_set_dropout in include/mdc.h states the
        counter-based mask generator)."""
        if topology.kind not in ("deployed", "cnnpy"):
            raise ValueError("the reference trains the deployed (CNN.ipynb cell 6) and cnn.py (cnn.py:104-112) nets; "
                             f"training is not built for {topology.kind!r}")
        self._open(device, _lib_variant)
        self.topology = topology
        self.layer_shapes, self.classes = topology.layer_shapes, topology.classes
        topo = _cabi.MdcTopology(_KIND[topology.kind], topology.filters, topology.hidden, topology.classes, (C.c_int32 * 4)(0, 0, 0, 0))
        self._check(self._fn("create")(C.byref(topo), self.device_index, C.byref(self._h)))
        self._set_adam(lr, beta1, beta2, eps)
        self.dropout, self.dropout_seed = float(dropout), int(dropout_seed) & 0xFFFFFFFF
        if self.dropout:
            self._check(self._fn("set_dropout")(self._h, self.dropout, self.dropout_seed))
        self._set(_cabi.TRAIN_WEIGHTS, weights)

    _frames = _TrainerCore._samples

    def evaluate(self, X, Y) -> float:
        """model.evaluate(X, Y): the mean categorical cross-entropy with the weights as they are now."""
        return self._evaluate(X, Y)["val_loss"]

    def save(self, filepath: str) -> None:
        """model.save(filepath) as ModelCheckpoint calls it (cnn.py:143): a Keras 2.4 full-model HDF5 file -- topology JSON,
        weights, training_config and Adam's state -- that the reference's model.load_weights(filepath) accepts."""
        from .formats.h5mini import write_keras_h5
        write_keras_h5(filepath, self.topology, self.get_weights(), optimizer=self.optimizer_state(), adam=self.adam)


class HeadTrainer(_TrainerCore):
    """Training state of a dense head on one MI355X (include/mdc.h, "head training"; csrc/head_train.hip): features K ->
    Dense(H, relu) -> Dense(C) -> softmax over precomputed f32 feature rows, the layers in front of them frozen.  VT-CNN2's head
    is (10560, 256, C) on the rows of `forward_device(tap="flat")`; `VTCNN2.fit_head` drives this class.  weights: [(W1 (K, H),
    b1 (H,)), (W2 (H, C), b2 (C,))] in Keras' layouts.  dropout = (rate in front of dense1, rate behind it), training batches only;
    mdc_trainer_set_dropout states the mask generator.  max_batch bounds the rows of one train_batch / evaluate call: all scratch
    is allocated for it here.  The history of fit also holds `val_accuracy`; this class knows the head only, so a checkpoint
    needs fit(save=)."""

    _PREFIX, _TRAIN_BATCH = "mdc_head_trainer_", "mdc_head_train_batch"
    _UNIT, _SAMPLES = "row", "features"
    _ALIGN16 = True
    _EXTRA = {"val_accuracy": "eval_correct"}

    def __init__(self, features: int, hidden: int, classes: int, weights: Sequence[Tuple[np.ndarray, np.ndarray]],
                 device: Optional[int] = None, max_batch: int = 1024, lr: float = 1e-3, beta1: float = 0.9, beta2: float = 0.999,
                 eps: float = 1e-7, dropout: Tuple[float, float] = (0.0, 0.0), dropout_seed: int = 0, _lib_variant: str = "product"):
        self._open(device, _lib_variant)
        self.features, self.hidden, self.classes, self.max_batch = int(features), int(hidden), int(classes), int(max_batch)
        self.layer_shapes = [((self.features, self.hidden), (self.hidden,)), ((self.hidden, self.classes), (self.classes,))]
        self._tail, self._max_rows = (self.features,), self.max_batch
        self._check(self._fn("create")(self.features, self.hidden, self.classes, self.max_batch, self.device_index, C.byref(self._h)))
        self._set_adam(lr, beta1, beta2, eps)
        self.dropout, self.dropout_seed = (float(dropout[0]), float(dropout[1])), int(dropout_seed) & 0xFFFFFFFF
        self._check(self._fn("set_dropout")(self._h, self.dropout[0], self.dropout[1], self.dropout_seed))
        if weights is not None:
            self._set(_cabi.TRAIN_WEIGHTS, weights)

    _rows = _TrainerCore._samples

    def evaluate(self, F, Y) -> Tuple[float, float]:
        """(mean categorical cross-entropy, accuracy) with the weights as they are now; no Dropout."""
        logs = self._evaluate(F, Y)
        return logs["val_loss"], logs["val_accuracy"]

