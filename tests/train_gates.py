"""Gates fixtures: batches on which the training kernels (csrc/train.hip) must take EVERY branch of their decision points.

The decision points (oracle/oracle_train.py states the rules, include/mdc.h promises them):
  * the clip of Keras' categorical_crossentropy: `q >= 1e-7 && q <= 1 - 1e-7`, per class;
  * the ReLU gates `pre > 0`, the deployed net's read-out `z > 0`, cnn.py's hidden layer `z1 > 0` -- at and below zero;
  * targets that are no one-hot rows (`y[c] != 0` per class);
  * cnn.py's padded operand tiles (columns past 3F, D and C; rows past a ragged batch);
  * Adam's update, away from its defaults and its first steps.

A fixture is ONE batch whose frames are drawn from a pool and SELECTED by what the f64 oracle computes on them, so each frame
is known to sit on a stated side of every decision, far enough from it that f32 and f64 cannot decide differently:

  interior      every q of the row in [1e-4, 1 - 1e-4]
  low / high    one-hot target whose class has q <= 1e-9 (loss term -log 1e-7, no gradient) / q >= 1 - 1e-9 (no gradient)
  silent        an all-zero frame under a zero conv bias: every conv pre-activation is exactly 0 and its gate must block
  dead          deployed: every z <= -0.1 (the read-out passes nothing; loss log 3).  cnn.py: at least one z1 <= -0.1, and one
                frame of the batch with all of them
  soft          0.9 onehot + 0.1 / C, a row summing to 2, an all-zero row; with three or more classes one smoothed row sits
                on a frame where one class with a non-zero target is clipped while another passes (two classes cannot do
                that: q0 <= 1e-7 means q1 >= 1 - 1e-7)

How saturation is reached.  Deployed nets: the frames are signal-shaped but live on an integer grid (7 bits, integer gains 1..3,
unit 2^-10) and the conv taps on quarters, so every conv pre-activation is an integer number of 2^-12 -- exactly 0 or at least
1 / 720 of the largest -- and the he_normal dense kernel is scaled by 1,500 (the read-out then spans +-60 and more); the
dense bias is (0.7, 0, -0.4): a silent frame puts z EXACTLY on 0 for class 1.  cnn.py's net: modulated_frames under per-frame
gains 75 .. 1200, its logit layer scaled until enough rows saturate; b1 cycles (0.5, 0, -0.3), so a silent frame has hidden
units above, on and below zero (a single hidden unit: exactly on zero).

`check_preconditions` proves all of this on the f64 oracle, and that the f32 numpy oracle stays within a quarter of the GPU
tests' bars on the fixture (an ill-conditioned fixture would otherwise show as a kernel failure).  A fixture that does not
meet them raises: a test ERROR, never a skip.

The MUTANTS are copies of the oracle's loss_and_grads_* and of KerasAdam.apply with one named fault each;
tests/test_train_gates.py shows on the CPU that every one of them leaves the true oracle by >= 100x the bar the GPU test
applies -- the evidence that tests/test_train_gates_gpu.py would notice a kernel with that fault.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

from modulationdetectioncnn_amd import Topology, synthetic_weights
from oracle import oracle_train as T
from tests.signals import modulated_frames

# the bars of tests/test_training_gpu.py: loss relative; gradients relative to the tensor's largest entry
LOSS_BAR, KERNEL_BAR, BIAS_BAR = 1e-5, 1e-5, 2e-5
Q_LOW, Q_HIGH = 1e-9, 1.0 - 1e-9
GREY_ZONES = ((1e-9, 1e-5), (1.0 - 1e-5, 1.0 - 1e-9))      # open intervals no q of a fixture may lie in
INTERIOR = (1e-4, 1.0 - 1e-4)
PASSES = (1e-5, 1.0 - 1e-5)
GATE_MARGIN = 1e-3                                         # no pre-activation within this fraction of its tensor's largest, except exact 0
DEAD = -0.1
MIN_PER_CATEGORY = 4
CATEGORIES = ("interior", "low", "high", "silent", "dead", "soft")

TOPOLOGIES = [("deployed", (3,)), ("deployed", (10,)), ("cnnpy", (10, 10, 5)), ("cnnpy", (1, 1, 2)), ("cnnpy", (5, 1, 16)), ("cnnpy", (6, 16, 2))]
TOPOLOGY_IDS = ["T1-F3", "T2-F10", "T4-10-10-5", "T4-1-1-2", "T4-5-1-16", "T4-6-16-2"]
MIXED_COUNTS = (93, 17)
PURE_COUNTS = (17, 48)
PURE_KINDS = ("low", "high", "dead", "silent")            # ('dead' as a pure batch: deployed only)
SILENT_EXACT_ZERO = (0, 1, 2)      # tensors (flat over (kernel, bias) pairs) whose gradient on all-silent frames is exactly 0: conv kernel, conv bias, first dense kernel


def topology_of(kind: str, shape) -> Topology:
    return Topology.deployed(shape[0], 3) if kind == "deployed" else Topology.cnnpy(*shape)


@dataclass
class Gates:
    kind: str
    shape: Tuple[int, ...]
    name: str
    weights: List[Tuple[np.ndarray, np.ndarray]]
    frames: np.ndarray                    # (n, 2, 128) f32
    targets: np.ndarray                   # (n, C) f32
    pure: Optional[str] = None            # None: a mixed batch; else the one category every frame belongs to

    @property
    def topology(self) -> Topology:
        return topology_of(self.kind, self.shape)


# ----------------------------------------------------------------------------------------------------------------------
# what the oracle decides on a batch (f64): the pre-activations in front of every gate and the clipped rows
# ----------------------------------------------------------------------------------------------------------------------
def trace(kind: str, x, weights, dtype=np.float64) -> Dict[str, np.ndarray]:
    """{'pre': (n, .) conv pre-activations, 'z': (n, .) the dense ReLU's (deployed z, cnn.py z1), 'q': (n, C)}, computed in `dtype`."""
    x = np.asarray(x, dtype)
    n = x.shape[0]
    if kind == "deployed":
        (ck, cb), (wd, bd) = [(np.asarray(k, dtype), np.asarray(b, dtype)) for k, b in weights]
        F = ck.shape[-1]
        k = ck.reshape(2, F)
        xp = np.zeros((n, 2, 130), dtype)
        xp[:, :, 1:129] = x
        pre = xp[:, :, 0:129, None] * k[0] + xp[:, :, 1:130, None] * k[1] + cb
        z = np.maximum(pre, 0).reshape(n, -1) @ wd + bd
        logits = np.maximum(z, 0)
    else:
        (ck, cb), (w1, b1), (w2, b2) = [(np.asarray(k, dtype), np.asarray(b, dtype)) for k, b in weights]
        F = ck.shape[-1]
        k = ck.reshape(2, 128, F)
        xp = np.zeros((n, 4, 128), dtype)
        xp[:, 1:3] = x
        pre = np.stack([xp[:, w] @ k[0] + xp[:, w + 1] @ k[1] for w in range(3)], axis=1) + cb
        z = np.maximum(pre, 0).reshape(n, -1) @ w1 + b1
        logits = np.maximum(z, 0) @ w2 + b2
    e = np.exp(logits - logits.max(axis=-1, keepdims=True))
    p = e / e.sum(axis=-1, keepdims=True)
    return {"pre": pre.reshape(n, -1), "z": z, "q": p / p.sum(axis=-1, keepdims=True)}


def _clear_of_zero(v: np.ndarray, scale: float) -> np.ndarray:
    """Per frame: every value is exactly 0 or further than GATE_MARGIN * scale from it."""
    return ((v == 0) | (np.abs(v) > GATE_MARGIN * scale)).all(axis=1)


def _no_grey(q: np.ndarray) -> np.ndarray:
    bad = np.zeros(q.shape, bool)
    for lo, hi in GREY_ZONES:
        bad |= (q > lo) & (q < hi)
    return ~bad.any(axis=1)


def _is_onehot(y: np.ndarray) -> np.ndarray:
    return ((y == 0) | (y == 1)).all(axis=1) & (y.sum(axis=1) == 1)


def membership(fx: Gates, tr: Optional[Dict[str, np.ndarray]] = None) -> Dict[str, np.ndarray]:
    """Boolean (n,) per category, from the f64 oracle's view of the batch.  Categories overlap: a silent frame is interior too."""
    tr = trace(fx.kind, fx.frames, fx.weights) if tr is None else tr
    q, y = tr["q"], fx.targets.astype(np.float64)
    hot = _is_onehot(y)
    qt = (q * y).sum(axis=1)                                   # the true class's q where the row is one-hot
    silent = (fx.frames == 0).all(axis=(1, 2)) & (tr["pre"] == 0).all(axis=1)
    dead = (tr["z"] <= DEAD).all(axis=1) if fx.kind == "deployed" else (tr["z"] <= DEAD).any(axis=1)
    return {"interior": ((q >= INTERIOR[0]) & (q <= INTERIOR[1])).all(axis=1), "low": hot & (qt <= Q_LOW), "high": hot & (qt >= Q_HIGH),
            "silent": silent, "dead": dead, "soft": ~hot}


# ----------------------------------------------------------------------------------------------------------------------
# pools: candidate frames with the oracle's trace on them, under the fixture's weights
# ----------------------------------------------------------------------------------------------------------------------
_DEP_DENSE_SCALE = 1500.0       # he_normal dense kernel x this: the read-out of the grid frames spans +-60 and more
_T4_GAINS = (75.0, 150.0, 300.0, 600.0, 1200.0)
_GRID_UNIT = 2.0 ** -10
_T4_SATURATED = 120


def _weights(kind: str, shape, seed: int):
    topo = topology_of(kind, shape)
    rng = np.random.default_rng(seed + 1000)
    w = [(k.copy(), b.copy()) for k, b in synthetic_weights(topo, seed=seed, bias_scale=0.05)]
    w[0] = (w[0][0], np.zeros_like(w[0][1]))                                   # a freshly initialised Keras conv: zero bias
    if kind == "deployed":
        w[0] = ((rng.choice([-3, -2, -1, 1, 2, 3], size=w[0][0].shape) / 4.0).astype(np.float32), w[0][1])
        w[1] = ((w[1][0] * _DEP_DENSE_SCALE).astype(np.float32), np.array([0.7, 0.0, -0.4], np.float32))
    else:
        D = shape[1]
        # b1 cycles (0.5, 0, -0.3); a single hidden unit sits exactly on zero (at 0.5 its scaled logit row would put the silent
        # frames' q into a grey zone)
        w[1] = (w[1][0], np.array([(0.5, 0.0, -0.3)[d % 3] for d in range(D)] if D > 1 else [0.0], np.float32))
    return w


def _pool_frames(kind: str, n: int, seed: int) -> np.ndarray:
    x, _lab, _snr = modulated_frames(n, seed=seed)
    rng = np.random.default_rng(seed + 1)
    if kind == "deployed":      # 7-bit signal-shaped integers (rms 12 units) x integer gain x 2^-10
        m = np.clip(np.rint(x.astype(np.float64) / 7.8e-3 * 12.0), -40, 40)
        return (m * rng.choice([1, 2, 3], size=n)[:, None, None] * _GRID_UNIT).astype(np.float32)
    return (x * rng.choice(_T4_GAINS, size=n)[:, None, None]).astype(np.float32)


Q_F32_DRIFT = 1e-6      # a frame on which the f32 forward pass alone moves a probability further than this is ill-conditioned


def _usable(tr) -> np.ndarray:
    return _no_grey(tr["q"]) & _clear_of_zero(tr["pre"], np.abs(tr["pre"]).max()) & _clear_of_zero(tr["z"], np.abs(tr["z"]).max())


@functools.lru_cache(maxsize=None)
def _pool(kind: str, shape, seed: int = 7):
    """-> (weights, frames, trace, usable): `usable` frames keep every gate clear of zero (against the POOL's scales, which bound
    any selection's) and every q out of the grey zones."""
    w = _weights(kind, shape, seed)
    x = _pool_frames(kind, 4000 if kind == "deployed" else 12000, seed)      # (the smallest cnn.py net keeps 1 frame in 250 as live interior)
    tr = trace(kind, x, w)
    if kind == "cnnpy":
        # the logit layer is scaled until _T4_SATURATED usable frames of the pool saturate (its he_normal init leaves every row
        # interior), and ONE designated frame gets all its hidden units dead: w1's columns change sign so that this frame's
        # projections are all negative (whole he_normal columns: the initialiser's distribution is symmetric)
        flat_sum = np.maximum(tr["pre"], 0).sum(axis=1)
        w1_0, w2_0 = w[1][0].copy(), w[2][0].copy()
        for i0 in np.argsort(-flat_sum)[:64]:
            proj = np.maximum(tr["pre"][i0], 0) @ w1_0.astype(np.float64)
            w[1] = ((w1_0 * np.where(proj > 0, -1.0, 1.0)).astype(np.float32), w[1][1])
            for step in range(60):
                w[2] = ((w2_0 * 1.25 ** step).astype(np.float32), w[2][1])
                t2 = trace(kind, x, w)
                if ((t2["q"].max(axis=1) >= Q_HIGH) & _usable(t2)).sum() >= _T4_SATURATED:
                    break
            if (t2["z"][i0] <= DEAD).all() and _usable(t2)[i0]:
                tr = t2
                break
        else:
            raise AssertionError(f"gates pool {kind}{shape}: no frame can be given all hidden units dead")
    drift = np.abs(trace(kind, x, w, np.float32)["q"].astype(np.float64) - tr["q"]).max(axis=1)
    return w, x, tr, _usable(tr) & (drift <= Q_F32_DRIFT)


def _candidates(kind: str, shape) -> Dict[str, np.ndarray]:
    """Pool indices per frame kind: I interior (live), SAT saturated, P partly clipped, D dead, AD all dead (cnn.py)."""
    w, x, tr, ok = _pool(kind, shape)
    q, z = tr["q"], tr["z"]
    interior = ((q >= INTERIOR[0]) & (q <= INTERIOR[1])).all(axis=1)
    sat = q.max(axis=1) >= Q_HIGH
    partly = (q <= Q_LOW).any(axis=1) & (((q >= PASSES[0]) & (q <= PASSES[1])).sum(axis=1) >= 2)
    if kind == "deployed":
        dead, live = (z <= DEAD).all(axis=1), (z > 0).any(axis=1)
        alldead = dead
    else:
        dead, live = interior & (z <= DEAD).any(axis=1), (z > 0).any(axis=1)
        alldead = (z <= DEAD).all(axis=1)
    pick = lambda m: np.nonzero(m & ok)[0]
    return {"I": pick(interior & live), "SAT": pick(sat), "P": pick(partly), "D": pick(dead), "AD": pick(alldead)}


# ----------------------------------------------------------------------------------------------------------------------
# builders
# ----------------------------------------------------------------------------------------------------------------------
# (frame kind, target kind) per batch position.  The periods are chosen against the kernels' strides: a deployed wave walks
# frames g, g + G, ... (G = ceil(n / 2) for 3 filters, ceil(n / 4) for 10: 47 / 24 at n = 93, 9 / 5 at n = 17), cnn.py's kernel takes
# 16 consecutive frames -- a period of 7 (and the 17-frame order below) puts different kinds into every wave and every tile.
_SOFT_CYCLE = [("P", "smooth"), ("I", "sum2"), ("I", "zero"), ("I", "smooth"), ("S", "smooth"), ("D", "sum2")]
_DEFAULT_TARGET = {"S": "hot", "I": "hot", "D": "hot", "P": "smooth"}


def _pattern(n: int):
    if n <= 17:
        cyc = [("S", "hot"), ("SAT", "low"), ("SAT", "high"), ("D", "hot")]
        out = [cyc[i % 4] for i in range(8)] + [("P", "smooth")] + [cyc[(i - 8) % 4] for i in range(9, 17)]
        out[4], out[3], out[11] = ("S", "smooth"), ("D", "sum2"), ("D", "zero")
        return out[:n]
    base = [("I", "hot"), ("SAT", "low"), ("SAT", "high"), ("S", "hot"), ("D", "hot"), None, ("P", "hot")]
    out, soft = [], 0
    for i in range(n):
        slot = base[i % len(base)]
        if slot is None:
            slot, soft = _SOFT_CYCLE[soft % len(_SOFT_CYCLE)], soft + 1
        elif slot[0] == "P" and (i // len(base)) % 2:      # (every other one: an interior frame -- the pools hold few partly clipped rows)
            slot = ("I", "hot")
        out.append(slot)
    return out


def _target(kind: str, q: np.ndarray, C: int, rng) -> np.ndarray:
    """A target row of the named kind for a frame whose oracle row is q."""
    y = np.zeros(C, np.float32)
    passing = np.nonzero((q >= PASSES[0]) & (q <= PASSES[1]))[0]
    if kind == "low":
        y[rng.choice(np.nonzero(q <= Q_LOW)[0])] = 1
    elif kind == "high":
        y[int(np.argmax(q))] = 1
    elif kind == "zero":
        pass
    else:
        lab = int(rng.choice(passing)) if len(passing) else int(rng.integers(C))
        y[lab] = 1
        if kind == "smooth":
            y = (np.float32(0.9) * y + np.float32(0.1 / C)).astype(np.float32)
        elif kind == "sum2":
            y[(lab + 1) % C] = 1
    return y


@functools.lru_cache(maxsize=None)
def mixed(kind: str, shape, n: int) -> Gates:
    """The mixed gates batch of n frames (n no multiple of 16), categories interleaved.  A selection on which the f32 numpy
    oracle leaves the f64 one by more than a quarter of the bars is ill-conditioned (a smoothed target next to its own q makes
    the one gradient a small batch has a difference of near-equal numbers): the next selection from the pool is taken."""
    for attempt in range(8):
        fx = _select_mixed(kind, tuple(shape), n, attempt)
        if not conditioning_faults(fx):
            return fx
    raise AssertionError(f"gates fixture {kind}{shape} n={n}: no well-conditioned selection in 8 attempts: {conditioning_faults(fx)}")


def _select_mixed(kind: str, shape, n: int, attempt: int) -> Gates:
    w, x, tr, _ok = _pool(kind, shape)
    cand = _candidates(kind, shape)
    C = tr["q"].shape[1]
    rng = np.random.default_rng(100 + n + 1000 * attempt)
    used: set = set()

    def take(name):
        for i in np.roll(cand[name], -11 * attempt if name != "AD" else 0):
            if int(i) not in used:
                used.add(int(i))
                return int(i)
        raise AssertionError(f"gates fixture {kind}{shape} n={n}: the pool has no unused '{name}' frame left ({len(cand[name])} in all)")

    silent_q = trace(kind, np.zeros((1, 2, 128), np.float32), w)["q"][0]
    frames, targets = [], []
    want_all_dead = kind == "cnnpy"
    for fk, tk in _pattern(n):
        if kind == "cnnpy" and C == 2 and fk == "P":
            fk = "I"                                      # two classes: no partly clipped row exists
        if fk == "S":
            frames.append(np.zeros((2, 128), np.float32))
            q = silent_q
        else:
            i = take("AD" if (fk == "D" and want_all_dead) else fk)
            if fk == "D":
                want_all_dead = False
            frames.append(x[i])
            q = tr["q"][i]
        targets.append(_target(tk, q, C, rng))
    return Gates(kind, tuple(shape), f"mixed-{n}", [(k.copy(), b.copy()) for k, b in w], np.stack(frames), np.stack(targets))


@functools.lru_cache(maxsize=None)
def pure(kind: str, shape, category: str, n: int) -> Gates:
    """n frames of ONE category: 'low', 'high', 'silent', or (deployed) 'dead'."""
    w, x, tr, _ok = _pool(kind, shape)
    cand = _candidates(kind, shape)
    C = tr["q"].shape[1]
    rng = np.random.default_rng(200 + n)
    if category == "silent":
        frames = np.zeros((n, 2, 128), np.float32)
        targets = T.onehot((np.arange(n) % 4 == 3).astype(np.int64), C)      # 3 : 1 classes 0 and 1 (labels in the proportion of the rows' own q would cancel in db)
    else:
        if category == "dead" and kind != "deployed":
            raise ValueError("an all-dead batch is a fixture of the deployed nets")
        idx = cand["D" if category == "dead" else "SAT"]
        if len(idx) < n:
            raise AssertionError(f"gates fixture {kind}{shape}: {len(idx)} '{category}' candidates in the pool, {n} needed")
        idx = idx[:n]
        frames = x[idx]
        targets = np.stack([_target("hot" if category == "dead" else category, tr["q"][i], C, rng) for i in idx])
    return Gates(kind, tuple(shape), f"pure-{category}-{n}", [(k.copy(), b.copy()) for k, b in w], frames, targets, pure=category)


# ----------------------------------------------------------------------------------------------------------------------
# preconditions
# ----------------------------------------------------------------------------------------------------------------------
def grad_errors(kind: str, got, ref) -> List[Tuple[str, float, float]]:
    """[(tensor name, error relative to the reference tensor's largest entry, bar)] over (kernel, bias) of every layer."""
    out = []
    for l, ((gk, gb), (rk, rb)) in enumerate(zip(got, ref)):
        for nm, g, r, bar in ((f"kernel{l}", gk, rk, KERNEL_BAR), (f"bias{l}", gb, rb, BIAS_BAR)):
            scale = float(np.abs(r).max())
            err = float(np.abs(np.asarray(g, np.float64) - r).max())
            out.append((nm, err / scale if scale > 0 else (0.0 if err == 0 else np.inf), bar))
    return out


def conditioning_faults(fx: Gates) -> List[str]:
    """Where the f32 numpy oracle leaves the f64 oracle by more than a QUARTER of the GPU tests' bars on this batch ([]: nowhere)."""
    l64, _a, g64, _b = T.loss_and_grads(fx.kind, fx.frames, fx.targets, fx.weights, np.float64)
    l32, _a, g32, _b = T.loss_and_grads(fx.kind, fx.frames, fx.targets, fx.weights, np.float32)
    out = [] if abs(l32 - l64) <= 0.25 * LOSS_BAR * abs(l64) else [f"f32 loss {l32!r} against {l64!r}"]
    return out + [f"the f32 oracle's {nm} is {err:.2e} from the f64 one (bar {bar:.0e})" for nm, err, bar in grad_errors(fx.kind, g32, g64) if not err <= 0.25 * bar]


def check_preconditions(fx: Gates) -> Dict[str, int]:
    """Raises AssertionError unless the f64 oracle confirms what the fixture claims.  -> frames per category."""
    tag = f"{fx.kind}{fx.shape} {fx.name}"
    n = len(fx.frames)
    assert fx.frames.dtype == np.float32 and fx.targets.dtype == np.float32 and fx.frames.shape == (n, 2, 128) and n <= 96, tag
    assert not np.any(fx.weights[0][1]), f"{tag}: the conv bias must be zero (silent frames)"
    tr = trace(fx.kind, fx.frames, fx.weights)
    _l, _li, _g, p = T.loss_and_grads(fx.kind, fx.frames, fx.targets, fx.weights, np.float64)
    assert np.allclose(tr["q"], p / p.sum(axis=-1, keepdims=True), rtol=1e-12, atol=1e-300), f"{tag}: trace() is not the oracle's forward"
    assert _no_grey(tr["q"]).all(), f"{tag}: a q lies in a grey zone of the clip"
    for nm in ("pre", "z"):
        assert _clear_of_zero(tr[nm], np.abs(tr[nm]).max()).all(), f"{tag}: a '{nm}' pre-activation lies within {GATE_MARGIN} of its scale of zero"
    mem = membership(fx, tr)
    counts = {c: int(mem[c].sum()) for c in CATEGORIES}
    y = fx.targets.astype(np.float64)
    if fx.pure is not None:
        assert mem[fx.pure].all(), f"{tag}: not every frame is '{fx.pure}' ({counts})"
        faults = conditioning_faults(fx) if fx.pure == "silent" else []      # (the other pure batches are held to exact zeros and the f32 oracle's loss)
        assert not faults, f"{tag}: ill-conditioned -- {faults}"
        return counts
    assert n % 16 != 0, tag
    for c in CATEGORIES:
        assert counts[c] >= MIN_PER_CATEGORY, f"{tag}: {counts[c]} '{c}' frames, {MIN_PER_CATEGORY} needed ({counts})"
    for s in range(0, n, 16):      # interleaved: every 16-frame tile of cnn.py's kernel holds several kinds
        kinds = sum(bool(mem[c][s:s + 16].any()) for c in CATEGORIES)
        assert kinds >= (3 if n - s >= 8 else 1), f"{tag}: the tile at {s} holds {kinds} categories"
    if fx.kind == "deployed":      # ... and so does every wave of the deployed kernels: frames g, g + G, ... (train.hip's waves_for)
        per_wave = 4 if fx.shape[0] == 10 else 2
        G_ = (n + per_wave - 1) // per_wave
        sig = np.stack([mem[c] for c in CATEGORIES], axis=1)
        for g in range(G_):
            rows = sig[g::G_]
            assert len(rows) < 2 or len({tuple(r) for r in rows}) >= 2, f"{tag}: wave {g} of {G_} walks frames of one kind only"
    C = y.shape[1]
    soft = mem["soft"]
    assert np.any(soft & np.isclose(y.sum(axis=1), 1.0) & (y > 0).all(axis=1)), f"{tag}: no label-smoothed row"
    assert np.any(soft & (y.sum(axis=1) == 2.0)) and np.any(soft & (y.sum(axis=1) == 0.0)), f"{tag}: no row summing to 2 / all-zero row"
    if C >= 3:
        q = tr["q"]
        clipped = (y != 0) & ((q <= Q_LOW) | (q >= Q_HIGH))
        passing = (y != 0) & (q >= PASSES[0]) & (q <= PASSES[1])
        assert np.any(soft & clipped.any(axis=1) & passing.any(axis=1)), f"{tag}: no soft row with one class clipped and another passing"
    if fx.kind == "cnnpy":
        assert np.any((tr["z"] <= DEAD).all(axis=1) & ~mem["silent"]), f"{tag}: no frame with every hidden unit dead"
    if fx.kind == "deployed":
        assert np.any(tr["z"][mem["silent"]] == 0), f"{tag}: no read-out exactly on zero"
    faults = conditioning_faults(fx)
    assert not faults, f"{tag}: ill-conditioned -- {faults}"
    return counts


def shuffled(fx: Gates, seed: int = 3, first: int = 5):
    """The same batch addressed through a shuffle: -> (resident frames, resident targets, order, first).  The resident set holds
    the fixture's frames in a random order, `order[first:first + n]` names them in the fixture's order again (in front of it:
    `first` other valid indices), so position i of the batch is frame order[first + i] of the data set -- the Dropout key."""
    n = len(fx.frames)
    perm = np.random.default_rng(seed).permutation(n)
    order = np.concatenate([perm[:first], np.argsort(perm)]).astype(np.int32)
    return fx.frames[perm], fx.targets[perm], order, first


DROPOUT_RATE = 0.5


@functools.lru_cache(maxsize=None)
def _dropout_seed(kind: str, shape, n: int) -> int:
    fx = mixed(kind, shape, n)
    _x, _y, order, first = shuffled(fx)
    for seed in range(1, 65):
        drop = dict(rate=DROPOUT_RATE, seed=seed, step=0, frames=order[first:])
        l64, _a, g64, p = T.loss_and_grads(kind, fx.frames, fx.targets, fx.weights, np.float64, dropout=drop)
        q = p / p.sum(axis=-1, keepdims=True)
        if ((q > 0.99e-7) & (q < 1.01e-7)).any():
            continue
        l32, _a, g32, _b = T.loss_and_grads(kind, fx.frames, fx.targets, fx.weights, np.float32, dropout=drop)
        if abs(l32 - l64) <= 0.25 * LOSS_BAR * abs(l64) and all(err <= 0.25 * bar for _nm, err, bar in grad_errors(kind, g32, g64)):
            return seed
    raise AssertionError(f"gates fixture {kind}{shape} n={n}: no Dropout seed in 1..64 keeps the masked batch well-conditioned")


def dropout_seed(fx: Gates) -> int:
    """The first Dropout seed under which the masked batch (rate 0.5, step 0, addressed through `shuffled`) is still decidable.
    The masks move the rows, so the fixture's own margins no longer hold; what must hold is that no q lies within 1 % of the
    clip's LOWER threshold -- there a class goes from no gradient to one of order 1, and f32 may decide differently -- and
    that the f32 numpy oracle stays within a quarter of the bars.  (At the upper threshold the gradient that passes or not is
    of order 1 - q = 1e-7 of a frame's share: far below any bar, whichever way f32 decides.)  The masks multiply the gates:
    DROP x blocked gates is a kernel path of its own."""
    return _dropout_seed(fx.kind, fx.shape, len(fx.frames))


# ----------------------------------------------------------------------------------------------------------------------
# mutants: oracle/oracle_train.py's loss_and_grads_* with ONE named fault (f64, no Dropout)
# ----------------------------------------------------------------------------------------------------------------------
XENT_FAULTS = ("clip_passes_everywhere", "clip_blocks_whole_row", "soft_targets_as_argmax")
GRAD_FAULTS = {"deployed": ("relu_ge_conv", "relu_ge_readout") + XENT_FAULTS + ("ragged_rows_in_bias_sums",),
               "cnnpy": ("relu_ge_conv", "relu_ge_hidden") + XENT_FAULTS + ("ragged_rows_in_bias_sums",)}
ADAM_FAULTS = ("eps_inside_root", "eps_hat_form", "v_from_g", "t_is_iterations")


def _mutant_xent(p, y, fault):
    if fault == "soft_targets_as_argmax":
        y = np.eye(y.shape[1])[y.argmax(axis=1)]
    eps = T.KERAS_EPSILON
    s = p.sum(axis=-1, keepdims=True)
    q = p / s
    qc = np.clip(q, eps, 1.0 - eps)
    loss = -(y * np.log(qc)).sum(axis=-1)
    passes = (q >= eps) & (q <= 1.0 - eps)
    if fault == "clip_passes_everywhere":
        passes = np.ones_like(passes)
    if fault == "clip_blocks_whole_row":
        passes = passes & passes.all(axis=-1, keepdims=True)
    gq = np.where(passes, -y / qc, 0.0)
    gp = (gq - (gq * q).sum(axis=-1, keepdims=True)) / s
    return loss, gp


def _gate(v, ge: bool):
    return (v >= 0) if ge else (v > 0)


def _mutant_deployed(x, y, weights, fault, n_mean):
    (ck, cb), (wd, bd) = weights
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    F = ck.shape[-1]
    k = np.asarray(ck, np.float64).reshape(2, F)
    b, wd, bd = (np.asarray(t, np.float64) for t in (cb, wd, bd))
    n = x.shape[0]
    xp = np.zeros((n, 2, 130))
    xp[:, :, 1:129] = x
    x0, x1 = xp[:, :, 0:129, None], xp[:, :, 1:130, None]
    pre = x0 * k[0] + x1 * k[1] + b
    flat = np.maximum(pre, 0).reshape(n, 258 * F)
    z = flat @ wd + bd
    p = T._softmax(np.maximum(z, 0))
    li, gp = _mutant_xent(p, y, fault)
    gz = T._softmax_backward(p, gp) * _gate(z, fault == "relu_ge_readout") / float(n_mean)
    dwd, dbd = flat.T @ gz, gz.sum(axis=0)
    ga = (gz @ wd.T).reshape(n, 2, 129, F) * _gate(pre, fault == "relu_ge_conv")
    dk = np.stack([(ga * x0).sum(axis=(0, 1, 2)), (ga * x1).sum(axis=(0, 1, 2))]).reshape(ck.shape)
    return li, [(dk, ga.sum(axis=(0, 1, 2))), (dwd, dbd)]


def _mutant_cnnpy(x, y, weights, fault, n_mean):
    (ck, cb), (w1, b1), (w2, b2) = weights
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    F = ck.shape[-1]
    k = np.asarray(ck, np.float64).reshape(2, 128, F)
    cb, w1, b1, w2, b2 = (np.asarray(t, np.float64) for t in (cb, w1, b1, w2, b2))
    n = x.shape[0]
    xp = np.zeros((n, 4, 128))
    xp[:, 1:3, :] = x
    pre = np.stack([xp[:, w] @ k[0] + xp[:, w + 1] @ k[1] for w in range(3)], axis=1) + cb
    flat = np.maximum(pre, 0).reshape(n, 3 * F)
    z1 = flat @ w1 + b1
    h = np.maximum(z1, 0)
    p = T._softmax(h @ w2 + b2)
    li, gp = _mutant_xent(p, y, fault)
    glg = T._softmax_backward(p, gp) / float(n_mean)
    dw2, db2 = h.T @ glg, glg.sum(axis=0)
    gz1 = (glg @ w2.T) * _gate(z1, fault == "relu_ge_hidden")
    dw1, db1 = flat.T @ gz1, gz1.sum(axis=0)
    ga = (gz1 @ w1.T).reshape(n, 3, F) * _gate(pre, fault == "relu_ge_conv")
    dk = np.zeros((2, 128, F))
    for w in range(3):
        dk[0] += xp[:, w].T @ ga[:, w]
        dk[1] += xp[:, w + 1].T @ ga[:, w]
    return li, [(dk.reshape(ck.shape), ga.sum(axis=(0, 1))), (dw1, db1), (dw2, db2)]


def mutant_loss_and_grads(kind: str, x, y, weights, fault: Optional[str]):
    """-> (mean loss, grads) of the f64 oracle with `fault` (None: the copy itself, which must equal the oracle bit for bit).
    'ragged_rows_in_bias_sums': the batch is padded to whole 16-frame tiles with zero frames that carry the last frame's (stale)
    target row, and those rows are summed into the BIAS gradients (the kernel gradients and the loss leave them out)."""
    fn = _mutant_deployed if kind == "deployed" else _mutant_cnnpy
    n = len(x)
    li, grads = fn(x, y, weights, fault, n)
    if fault == "ragged_rows_in_bias_sums":
        pad = (-n) % 16
        xpad = np.concatenate([np.asarray(x, np.float64), np.zeros((pad, 2, 128))])
        ypad = np.concatenate([np.asarray(y, np.float64), np.repeat(np.asarray(y, np.float64)[-1:], pad, axis=0)])
        _li, gpad = fn(xpad, ypad, weights, None, n)
        grads = [(gk, gbp) for (gk, _gb), (_gkp, gbp) in zip(grads, gpad)]
    return float(li.mean(dtype=np.float64)), grads


# ----------------------------------------------------------------------------------------------------------------------
# one Adam update, isolated from the gradient
# ----------------------------------------------------------------------------------------------------------------------
ADAM_CASES = {"defaults": dict(T.ADAM_DEFAULTS), "all-changed": dict(lr=1e-2, beta1=0.5, beta2=0.9, eps=1e-3),
              "beta1-zero": dict(T.ADAM_DEFAULTS, beta1=0.0)}
ADAM_ITERATIONS = (0, 1, 950, 100000)      # 950: the `iter` of the bundled checkpoints
ADAM_WEIGHT_SCALE = 2.0 ** -5
ADAM_TOPOLOGIES = [("deployed", (3,)), ("deployed", (10,)), ("cnnpy", (10, 10, 5)), ("cnnpy", (6, 16, 2))]


def adam_fixture(kind: str, shape, batch: str) -> Gates:
    """17 frames for one isolated update, under freshly initialised weights scaled by 2^-5 (zero conv bias).  Small weights on
    purpose: w' = fl(w - dw) carries up to an ulp of w whatever the update's arithmetic does, and the bar on dw is a few 1e-7 of
    the tensor's largest step -- at |w| ~ 1 and steps ~ lr the weight's own rounding would be as large as the bar
    (`adam_rounding_clearance` is asserted before a result is looked at).
    batch 'silent': all-zero frames, the gradient of every tensor in front of the last bias-fed layer is exactly 0;
    batch 'signal': modulated frames, no gradient is 0."""
    topo = topology_of(kind, shape)
    w = [((k * ADAM_WEIGHT_SCALE).astype(np.float32), (b * ADAM_WEIGHT_SCALE).astype(np.float32)) for k, b in synthetic_weights(topo, seed=21, bias_scale=0.05)]
    w[0] = (w[0][0], np.zeros_like(w[0][1]))
    x, lab, _snr = modulated_frames(17, seed=5)
    if batch == "silent":
        x = np.zeros_like(x)
    elif kind == "cnnpy":
        x = (x * 40.0).astype(np.float32)
    return Gates(kind, tuple(shape), f"adam-{batch}", w, x, T.onehot(lab % topo.classes, topo.classes))


def adam_moments(shapes, seed: int, zero: Tuple[int, ...] = ()):
    """Random first moments of both signs and second moments >= 0 spread over ten decades (sqrt(v) from Adam's epsilon up); every
    tensor's first element has v = 0 under a large m (the tensor's largest step, which the bar on dw is relative to),
    its second a negative m under the largest v.  The tensors listed in `zero` get m = v = 0."""
    rng = np.random.default_rng(seed)
    m = [(rng.standard_normal(s) * 0.05).astype(np.float32) for s in shapes]
    v = [(10.0 ** rng.uniform(-14.0, -4.0, size=s)).astype(np.float32) for s in shapes]
    for mi, vi in zip(m, v):
        mi.reshape(-1)[0], vi.reshape(-1)[0] = 0.05, 0.0
        if mi.size > 1:
            mi.reshape(-1)[1], vi.reshape(-1)[1] = -0.05, 1e-4
    for i in zero:
        m[i][...] = 0
        v[i][...] = 0
    return m, v


def adam_step(w, g, m, v, iterations: int, hyper: dict, fault: Optional[str] = None):
    """-> (w', m', v') as f32 lists.  fault None: oracle_train.KerasAdam itself; else its apply() with that one fault."""
    w, m, v = ([np.array(t, np.float32) for t in ts] for ts in (w, m, v))
    g = [np.asarray(t, np.float32) for t in g]
    if fault is None:
        opt = T.KerasAdam([t.shape for t in w], **hyper)
        opt.m, opt.v, opt.iterations = m, v, int(iterations)
        opt.apply(w, g)
        assert opt.iterations == iterations + 1
        return w, opt.m, opt.v
    f = np.float32
    lr, beta1, beta2, eps = (f(hyper[k]) for k in ("lr", "beta1", "beta2", "eps"))
    t = iterations if fault == "t_is_iterations" else iterations + 1
    with np.errstate(all="ignore"):
        b1p, b2p = f(np.power(beta1, f(t))), f(np.power(beta2, f(t)))
        alpha = f(lr * np.sqrt(f(1) - b2p) / (f(1) - b1p))
        for p, gi, mi, vi in zip(w, g, m, v):
            mi += (gi - mi) * (f(1) - beta1)
            vi += ((gi if fault == "v_from_g" else gi * gi) - vi) * (f(1) - beta2)
            if fault == "eps_inside_root":
                p -= (mi * alpha) / np.sqrt(vi + eps)
            elif fault == "eps_hat_form":      # torch / the paper: m^ / (sqrt(v^) + eps)
                p -= (lr * mi / (f(1) - b1p)) / (np.sqrt(vi / (f(1) - b2p)) + eps)
            else:
                p -= (mi * alpha) / (np.sqrt(vi) + eps)
    return w, m, v


def adam_bars(m, v, g, dw_ref, iterations: int, hyper: dict):
    """The bars of one update against KerasAdam in f32: m' and v' element-wise (the kernel may contract m + (g - m)(1 - b1) into
    one fma), and dw = w' - w relative to the oracle's largest step: one ulp of 1 in each of the two powers of alpha (divided by
    what 1 - beta^t leaves of it) plus eight ulps for sqrtf, the division and the products."""
    u = 2.0 ** -24
    t = iterations + 1
    b1, b2 = float(np.float32(hyper["beta1"])), float(np.float32(hyper["beta2"]))
    m, v, g = (np.asarray(a, np.float64) for a in (m, v, g))
    rel = u / (1.0 - b2 ** t) + 2.0 * u / (1.0 - b1 ** t) + 8.0 * u
    return 4.0 * u * (np.abs(m) + np.abs(g)), 4.0 * u * (v + g * g), 4.0 * rel * float(np.abs(np.asarray(dw_ref, np.float64)).max())


def adam_rounding_clearance(w, bar_dw: float) -> float:
    """How many times an ulp of the tensor's largest weight fits into the bar on dw (the tests ask for >= 4)."""
    return bar_dw / (2.0 ** -23 * float(np.abs(w).max())) if np.any(w) else np.inf
