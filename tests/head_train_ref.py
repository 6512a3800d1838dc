"""Reference of head training (include/mdc.h, "head training"): features K -> Dense(H, relu) -> Dense(C) -> softmax with
Keras 2.4's categorical cross-entropy on the softmax output and TensorFlow 2.4's Adam, in numpy (float64 unless told
otherwise).  TEST INFRASTRUCTURE ONLY.  The loss, the Dropout generator and Adam are oracle/oracle_train.py's;
tests/test_head_train_ref.py holds this file to torch autograd in f64.

Also the fixtures of the GPU tests: features max(0, N(0, 1)) * 0.05 (about half zeros, as conv2 + ReLU gives), Glorot
kernels, every value rounded to f32 before either precision sees it, and rows selected ON THE F64 REFERENCE ALONE so that
no hidden pre-activation lies so close to zero that f32 rounding could flip its ReLU gate."""
from __future__ import annotations

import functools
from typing import Dict, List, Optional, Tuple

import numpy as np

from oracle.oracle_train import KerasAdam, crossentropy_on_probs, dropout_scale

Weights = List[Tuple[np.ndarray, np.ndarray]]
SHAPES = [(10560, 256, 11, 93), (10560, 256, 11, 1), (10560, 256, 11, 257), (96, 32, 2, 17), (32, 32, 16, 50)]      # (K, H, C, count)
GUARD = 1e-5          # a row is dropped if any |z1| < GUARD * max|z1| and z1 is not exactly 0
MAX_DROPPED = 0.05    # of the pool


def _softmax(z):
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def scales(dropout: Optional[dict], n: int, K: int, H: int, dtype):
    """(s0, s1): keep / (1 - rate) per feature and per hidden unit; dropout = {'rates': (r0, r1), 'seed', 'step', 'frames'}."""
    s0 = s1 = None
    if dropout is not None:
        r0, r1 = dropout["rates"]
        if r0 > 0:
            s0 = dropout_scale(r0, dropout["seed"], dropout["step"], dropout["frames"], K, 0, dtype)
        if r1 > 0:
            s1 = dropout_scale(r1, dropout["seed"], dropout["step"], dropout["frames"], H, 1, dtype)
    return s0, s1


def forward(f, weights: Weights, dtype=np.float64, dropout: Optional[dict] = None) -> Dict:
    (w1, b1), (w2, b2) = [(np.asarray(k, dtype), np.asarray(b, dtype)) for k, b in weights]
    f = np.asarray(f, dtype)
    s0, s1 = scales(dropout, f.shape[0], w1.shape[0], w1.shape[1], dtype)
    a = f if s0 is None else f * s0
    z1 = a @ w1 + b1
    h = np.maximum(z1, 0)
    if s1 is not None:
        h = h * s1
    z2 = h @ w2 + b2
    return dict(a=a, z1=z1, h=h, z2=z2, p=_softmax(z2), s1=s1, w2=w2)


def loss_and_grads(f, y, weights: Weights, dtype=np.float64, dropout: Optional[dict] = None, divide_by: Optional[int] = None):
    """(mean loss, per-row losses, [(dW1, db1), (dW2, db2)] of the MEAN loss, probabilities).  divide_by: the batch's `count`
    when some of its positions were skipped (the mean still divides by count)."""
    y = np.asarray(y, dtype)
    fw = forward(f, weights, dtype, dropout)
    n = dtype(divide_by if divide_by is not None else len(y))
    li, gp = crossentropy_on_probs(fw["p"], y)
    p = fw["p"]
    dz2 = p * (gp - (gp * p).sum(axis=-1, keepdims=True)) / n
    dh = dz2 @ fw["w2"].T
    if fw["s1"] is not None:
        dh = dh * fw["s1"]
    dz1 = dh * (fw["z1"] > 0)
    grads = [(fw["a"].T @ dz1, dz1.sum(axis=0)), (fw["h"].T @ dz2, dz2.sum(axis=0))]
    return float(li.sum(dtype=np.float64) / float(n)), li, grads, p


def evaluate(f, y, weights: Weights, dtype=np.float64) -> Tuple[float, int]:
    """(loss sum, rows whose arg-max of p equals the arg-max of the target row; the lowest index on a tie, both sides)."""
    fw = forward(f, weights, dtype)
    li, _ = crossentropy_on_probs(fw["p"], np.asarray(y, dtype))
    return float(li.sum(dtype=np.float64)), int((fw["p"].argmax(axis=1) == np.asarray(y).argmax(axis=1)).sum())


def flat(weights: Weights) -> List[np.ndarray]:
    return [t for pair in weights for t in pair]


def train_step(f, y, weights: Weights, opt: KerasAdam, dtype=np.float64, dropout: Optional[dict] = None) -> float:
    """Gradients in `dtype`, then KerasAdam's f32 update of the f32 weights IN PLACE; dropout = {'rates', 'seed', 'frames'}."""
    if dropout is not None:
        dropout = dict(dropout, step=opt.iterations)
    loss, _li, grads, _p = loss_and_grads(f, y, weights, dtype, dropout)
    opt.apply(flat(weights), flat(grads))
    return loss


def fit(weights: Weights, f, y, batch_size: int, epochs: int, validation_data, permutations, dtype=np.float64) -> Dict:
    """HeadTrainer.fit's loop without callbacks: {'loss', 'val_loss', 'val_accuracy', 'weights'}."""
    weights = [(k.astype(np.float32).copy(), b.astype(np.float32).copy()) for k, b in weights]
    opt = KerasAdam([t.shape for t in flat(weights)])
    fv, yv = validation_data
    hist = {"loss": [], "val_loss": [], "val_accuracy": []}
    for ep in range(epochs):
        order, tot = permutations(ep), 0.0
        for s in range(0, len(f), batch_size):
            idx = order[s:s + batch_size]
            tot += train_step(f[idx], y[idx], weights, opt, dtype) * len(idx)
        hist["loss"].append(tot / len(f))
        ls, hits = evaluate(fv, yv, weights, dtype)
        hist["val_loss"].append(ls / len(fv))
        hist["val_accuracy"].append(hits / len(fv))
    hist["weights"] = weights
    return hist


# ---- fixtures ----------------------------------------------------------------------------------------------------------------
def glorot_weights(K: int, H: int, C: int, seed: int, bias_scale: float = 0.01) -> Weights:
    rng = np.random.default_rng(seed)
    l1, l2 = np.sqrt(6.0 / (K + H)), np.sqrt(6.0 / (H + C))
    return [(rng.uniform(-l1, l1, (K, H)).astype(np.float32), (bias_scale * rng.standard_normal(H)).astype(np.float32)),
            (rng.uniform(-l2, l2, (H, C)).astype(np.float32), (bias_scale * rng.standard_normal(C)).astype(np.float32))]


def feature_rows(n: int, K: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return (np.maximum(rng.standard_normal((n, K)), 0.0) * 0.05).astype(np.float32)


def target_rows(n: int, C: int, seed: int) -> np.ndarray:
    """One-hot rows, every third one a general distribution (f32 values; the rows need not sum to 1 exactly).  Class c is drawn
    with weight c + 1: with even classes and a fresh head, db2 = mean(p) - mean(y) is a sum that cancels to nearly nothing, and
    a bar relative to its largest entry would then measure the cancellation, not the arithmetic."""
    rng = np.random.default_rng(seed)
    y = np.zeros((n, C), np.float32)
    y[np.arange(n), rng.choice(C, n, p=np.arange(1, C + 1) / (C * (C + 1) / 2))] = 1.0
    soft = rng.dirichlet(np.ones(C), n).astype(np.float32)
    y[::3] = soft[::3]
    return y


def guarded(z1: np.ndarray) -> np.ndarray:
    """Rows the f32 kernels can be held to the f64 reference on: no hidden pre-activation within GUARD of zero, unless exactly 0."""
    near = (np.abs(z1) < GUARD * np.abs(z1).max()) & (z1 != 0)
    return ~near.any(axis=1)


class Fixture:
    """A pool of feature rows (the device buffer of the `order` and Dropout runs), targets, weights, and the positions the
    guard keeps: `keep` without Dropout, `keep_drop` with `dropout` at step 0 (frame = the row's index in the pool)."""

    def __init__(self, K: int, H: int, C: int, count: int, seed: int = 0):
        self.K, self.H, self.C, self.count = K, H, C, count
        self.pool = count + max(4, (count + 15) // 16)
        self.f = feature_rows(self.pool, K, 100 + seed)
        self.y = target_rows(self.pool, C, 200 + seed)
        self.w = glorot_weights(K, H, C, 300 + seed)
        self.dropout = dict(rates=(0.5, 0.5), seed=77 + seed, step=0, frames=np.arange(self.pool))
        self.keep = self._select(forward(self.f, self.w)["z1"])
        self.keep_drop = self._select(forward(self.f, self.w, dropout=self.dropout)["z1"])

    def _select(self, z1: np.ndarray) -> np.ndarray:
        ok = np.flatnonzero(guarded(z1))
        if self.pool - len(ok) > MAX_DROPPED * self.pool or len(ok) < self.count:
            raise AssertionError(f"the guard dropped {self.pool - len(ok)} of {self.pool} rows: more than {MAX_DROPPED:.0%}, or too few left")
        return ok[:self.count]


@functools.lru_cache(maxsize=None)
def fixture(K: int, H: int, C: int, count: int, seed: int = 0) -> Fixture:
    return Fixture(K, H, C, count, seed)


def rel(a, b) -> float:
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / max(float(np.abs(b).max()), 1e-300))


@functools.lru_cache(maxsize=None)
def adam_case(with_dropout: bool, K: int = 10560, H: int = 256, C: int = 11, rows: int = 176, batch: int = 64, steps: int = 20, seed: int = 5) -> Dict:
    """20 steps of batch 64 over 176 rows: step i trains on order[64 i : 64 (i + 1)], `order` being shuffles of the rows back to
    back.  'ref': the weights after the f64 reference's steps, 'moved': max|w - w0| per tensor of that trajectory."""
    rng = np.random.default_rng(seed)
    f, y, w0 = feature_rows(rows, K, 400 + seed), target_rows(rows, C, 500 + seed), glorot_weights(K, H, C, 600 + seed)
    order = np.concatenate([rng.permutation(rows) for _ in range((steps * batch + rows - 1) // rows)])[:steps * batch].astype(np.int32)
    dropout = dict(rates=(0.5, 0.5), seed=31) if with_dropout else None
    w = [(k.copy(), b.copy()) for k, b in w0]
    opt = KerasAdam([t.shape for t in flat(w)])
    losses = []
    for i in range(steps):
        idx = order[i * batch:(i + 1) * batch]
        losses.append(train_step(f[idx], y[idx], w, opt, np.float64, None if dropout is None else dict(dropout, frames=idx)))
    moved = [float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(flat(w), flat(w0))]
    return dict(f=f, y=y, w0=w0, order=order, batch=batch, steps=steps, dropout=dropout, ref=w, moved=moved, losses=losses)
