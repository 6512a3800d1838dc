"""Exact-integer fixtures: inputs on which every precision mode must equal the f64 oracle BIT FOR BIT.

Weights and frames are small integers times a power of two (the unit U = 2^-7).  Every product and every partial sum of
every layer is then an integer number of units far below 2^24, i.e. exact in f32 in ANY accumulation order, and the
library's internal scales (2^-32 of the clamp-bit ReLU, the fp8 activation / weight / feature scales, 2^+32 on the dense
weights) are exact powers of two.  What is left of a reduced-precision mode is its narrowing conversions, which
`expected()` restates on top of oracle/oracle_np.py, called layer by layer in f64.  `check_preconditions()` proves on the
oracle alone that a fixture has these properties before a GPU result is looked at.

NARROWING POINTS (paths below modulationdetectioncnn_amd/csrc/; each is one `t.narrow` call in `expected()`):
  vtcnn2 bf16 / fp8   frames as bf16 hi + bf16 lo             vtcnn2_bf16_common.h:83-85, vtcnn2_sched_common.h:140-142
                      conv1 taps and bias as bf16 hi + lo      vtcnn2_bf16.hip:304-311, vtcnn2_bf16_sched.hip:452-459,
                                                               vtcnn2_fp8_conv.hip:502-509
                      conv2 weights  bf16: f2bf                vtcnn2_bf16.hip:291, vtcnn2_bf16_sched.hip:439
                                     fp8:  f2e4m3(w 2^sw)      vtcnn2_fp8_conv.hip:491 (sw: :474)
                      conv1 activations  bf16: v_cvt_pk_bf16_f32 (RNE) + ReLU    vtcnn2_bf16.hip:145, vtcnn2_bf16_sched.hip:112
                                         fp8: bf16 as above, then v_cvt_scalef32_pk_fp8_bf16 (RNE, e4m3 of a 2^sa)
                                                               vtcnn2_fp8_conv.hip:112, :117 (sa: :475)
                      conv2 features     bf16 (and fp8 with fp8_bf16_features): v_cvt_pk_bf16_f32
                                                               vtcnn2_bf16.hip:180-183, vtcnn2_sched_common.h:104-111
                                         fp8: v_cvt_scalef32_pk_fp8_f32 (RNE, e4m3 of v 2^kf, ONE rounding from f32)
                                                               vtcnn2_fp8_conv.hip:132-144 (kf: :548)
                      dense1 weights bf16                      vtcnn2_bf16.hip:336, vtcnn2_fp8_conv.hip:560
                      (dense1's bias, the hidden layer, dense2 and the softmax stay f32: vtcnn2_bf16_dense1.hip:167, :191-198)
  deployed bf16       conv outputs v_cvt_pk_bf16_f32           deployed_bf16.hip:88;   dense weights f2bf  :513
  deployed f16        frames, taps, bias, conv outputs in f16  deployed_bf16.hip:156-158, :317, :324; dense weights f2h :513
  deployed fp8        conv outputs e4m3 of y 2^sa, ONE rounding from f32   deployed_bf16.hip:102-103 (sa, sw: :530);
                      dense weights f2e4m3_sat(w 2^sw)         :512
  f32 (all kinds), cnn.py's net: no narrowing point.
All conversions are round-to-nearest-even; the e4m3 ones saturate at 448 (MODE.FP16_OVFL), which no fixture reaches.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

from oracle import oracle_np as O

U = 2.0 ** -7                      # the unit: every fixture value is an integer times U (taps: plain integers)
EXACT_F32 = float(2 ** 24)         # sum |term| below this many units: every partial sum is an f32 integer
VT_MODES = [("f32", False), ("bf16", False), ("fp8", False), ("fp8", True)]      # (dtype, fp8_bf16_features)
DEP_MODES = ["f32", "bf16", "f16", "fp8"]


# ----------------------------------------------------------------------------------------------------------------------
# narrowing functions (f64 in, f64 out; `trunc` = round toward zero instead of to nearest even: the sensitivity check's fault)
# ----------------------------------------------------------------------------------------------------------------------
def narrow_bf16(a, trunc: bool = False) -> np.ndarray:
    """f32 -> bf16, round to nearest even (v_cvt_pk_bf16_f32; host f2bf, vtcnn2_bf16_common.h:121-127)."""
    u = np.ascontiguousarray(a, np.float64).astype(np.float32).view(np.uint32).astype(np.uint64)
    if not trunc:
        u = u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))
    u = (u & np.uint64(0xFFFF0000)).astype(np.uint32)
    return u.view(np.float32).astype(np.float64).reshape(np.shape(a))


def narrow_bf16_split(a) -> np.ndarray:
    """The 16-bit modes' frames and conv1 operands: bf16 hi + bf16(x - hi) lo, both halves multiplied out."""
    hi = narrow_bf16(a)
    return hi + narrow_bf16(np.asarray(a, np.float64) - hi)


def narrow_f16(a, trunc: bool = False) -> np.ndarray:
    """f32 -> IEEE f16, round to nearest even (host f2h, deployed_bf16.hip:446-467; the (_Float16) casts of the kernel)."""
    a = np.asarray(a, np.float64)
    r = a.astype(np.float32).astype(np.float16).astype(np.float64)
    if trunc:
        over = np.abs(r) > np.abs(a)
        r = np.where(over, np.nextafter(r.astype(np.float16), np.float16(0)).astype(np.float64), r)
    return r


def narrow_e4m3(a, trunc: bool = False) -> np.ndarray:
    """-> OCP e4m3 "fn": 4 significant bits, round to nearest even, subnormals below 2^-6 on the 2^-9 grid, saturating at 448
    (host f2e4m3, vtcnn2_fp8_conv.hip:441-457; v_cvt_scalef32_pk_fp8_* under MODE.FP16_OVFL)."""
    a = np.asarray(a, np.float64)
    mag = np.abs(a)
    _, e = np.frexp(mag)                                  # mag = m 2^e, m in [0.5, 1)
    E = np.maximum(e - 1, -6)                             # mag = 1.xxx 2^E; subnormals share E = -6
    q = np.ldexp(mag, 3 - E)                              # 3 fraction bits kept
    q = np.floor(q) if trunc else np.rint(q)              # np.rint: half to even
    return np.copysign(np.minimum(np.ldexp(q, E - 3), 448.0), a)


def is_e4m3_tie(a) -> np.ndarray:
    """True where rounding `a` to e4m3 is a genuine half-way case."""
    mag = np.abs(np.asarray(a, np.float64))
    _, e = np.frexp(mag)
    q = np.ldexp(mag, 3 - np.maximum(e - 1, -6))
    return (q - np.floor(q)) == 0.5


NARROW = {"bf16": narrow_bf16, "f16": narrow_f16, "e4m3": narrow_e4m3, "bf16x2": lambda a, trunc=False: narrow_bf16_split(a)}
_MIN_NORMAL = {"bf16": 2.0 ** -126, "bf16x2": 2.0 ** -126, "f16": 2.0 ** -14, "e4m3": 2.0 ** -6}
_MAX_FINITE = {"bf16": 3.38e38, "bf16x2": 3.38e38, "f16": 65504.0, "e4m3": 448.0}


# ----------------------------------------------------------------------------------------------------------------------
# fixtures
# ----------------------------------------------------------------------------------------------------------------------
@dataclass
class Fixture:
    kind: str                                  # 'vtcnn2' | 'deployed' | 'cnnpy'
    shape: Tuple[int, ...]                     # vtcnn2 (C,); deployed (F, C); cnnpy (F, D, C)
    flavour: str                               # 'dense' | 'sparse'
    weights: List[Tuple[np.ndarray, np.ndarray]]
    frames: np.ndarray                         # (n, 2, 128) f32
    tie_pair: Optional[Tuple[int, int]] = None
    fp8_input_absmax: float = U
    fp8_feature_absmax: Optional[float] = None

    @property
    def flat_weights(self):
        return [a for p in self.weights for a in p]


def _ternary(rng, shape, density):
    return rng.choice([-1.0, 1.0], size=shape) * (rng.random(shape) < density)


def _signs(rng, n, mags):
    """n non-zero values of both signs with magnitudes drawn from `mags`."""
    b = rng.choice(mags, size=n) * rng.choice([-1.0, 1.0], size=n)
    if n >= 2:
        b[0], b[1] = abs(b[0]), -abs(b[1])
    return b


def fixture_frames(n: int, seed: int, amp: int = 1) -> np.ndarray:
    """Frame 0 all zero; frames 1..4 one-sample impulses at the four row ends (row 0 sample 0 / 127, row 1 sample 0 / 127: the
    padded positions w = 0, 1, 130, 131 of VT-CNN2, w = 0 and 128 of the deployed nets); frame 5 an impulse in the middle; the
    rest integers in [-amp, amp] times U."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-amp, amp + 1, size=(n, 2, 128)).astype(np.float64) * U
    edge = [(0, 0), (0, 127), (1, 0), (1, 127), (0, 63)]
    for i in range(min(n, 6)):
        x[i] = 0.0
        if i >= 1:
            h, s = edge[i - 1]
            x[i, h, s] = U if i % 2 else -U
    return x.astype(np.float32)


def _pow2_at_least(v: float) -> float:
    return float(2.0 ** np.ceil(np.log2(v)))


def _spread_dense2(logits_max: float) -> float:
    """Power of two that brings the largest |logit| into [4, 8): the softmax rows are neither uniform nor one-hot everywhere."""
    return float(2.0 ** (2 - np.floor(np.log2(logits_max)))) if logits_max > 0 else 1.0


def _tie_columns(k, b, pair):
    if pair is not None:
        k[:, pair[1]] = k[:, pair[0]]
        b[pair[1]] = b[pair[0]]


def _draw_head(hid, classes, key, draw):
    """The last Dense layer: `draw(rng)` gives its kernel; redrawn (sub-seeds 0, 1, ...) until the plain oracle's labels take at
    least min(4, classes) values with the tied pair in place.  The pair is the most frequent winner copied over a class that never
    wins, so it is the maximum of some frames.  Returns kernel, bias, pair, logits."""
    for sub in range(256):
        r2 = np.random.default_rng(list(map(int, key)) + [sub, 77])
        w2 = draw(r2)
        c2 = _signs(r2, classes, [1.0, 2.0, 3.0]) * U
        wins = np.bincount(O.argmax_first(O.dense(hid, w2, c2, False, np.float64)), minlength=classes)
        never = np.flatnonzero(wins == 0)
        pair = None
        if classes >= 3 and never.size:
            top = int(np.argmax(wins))
            other = int(never[0])
            pair = (min(top, other), max(top, other))
            w2[:, other], c2[other] = w2[:, top], c2[top]
        lg = O.dense(hid, w2, c2, False, np.float64)
        if len(np.unique(O.argmax_first(lg))) >= min(4, classes) and (pair is not None or classes < 3):
            return w2, c2, pair, lg
    raise AssertionError(f"no dense2 draw gives four labels and a tied maximum (key {key})")


def vtcnn2_fixture(classes: int, flavour: str, seed: int = 0, nframes: int = 64) -> Fixture:
    """The dense2 draw is repeated (sub-seeds 0, 1, ...) until the plain oracle's labels take at least four values with the
    tied pair in place; the pair is the most frequent winner copied over a class that never wins, so it is some frames' maximum."""
    rng = np.random.default_rng([seed, classes, flavour == "dense"])
    k1 = rng.integers(-1, 2, size=(256, 1, 1, 3)).astype(np.float64)
    b1 = _signs(rng, 256, [1.0]) * U
    if flavour == "dense":
        k2 = _ternary(rng, (80, 256, 2, 3), 0.25)
    else:
        k2 = np.zeros((80, 1536))
        for o in range(80):
            k2[o, rng.choice(1536, size=3, replace=False)] = rng.choice([-1.0, 1.0], size=3)
        k2 = k2.reshape(80, 256, 2, 3)
    b2 = _signs(rng, 80, [1.0, 2.0]) * U
    w1 = _ternary(rng, (10560, 256), 0.5)
    c1 = _signs(rng, 256, [1.0, 2.0, 3.0]) * U
    x = fixture_frames(nframes, seed + 1)
    flat = O.vtcnn2_conv2(O.vtcnn2_conv1(x, k1, b1, np.float64), k2, b2, np.float64).reshape(nframes, -1)
    hid = O.dense(flat, w1, c1, True, np.float64)
    w2, c2, pair, lg = _draw_head(hid, classes, [seed, classes, flavour == "dense"], lambda r: _ternary(r, (256, classes), 0.75))
    s = _spread_dense2(float(np.abs(lg).max()))
    w2, c2 = w2 * s, c2 * s
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    fx = Fixture("vtcnn2", (classes,), flavour, [(f32(k1), f32(b1)), (f32(k2), f32(b2)), (f32(w1), f32(c1)), (f32(w2), f32(c2))], x, pair)
    fx.fp8_input_absmax = _pow2_at_least(float(np.abs(x).max()))
    fx.fp8_feature_absmax = _pow2_at_least(float(flat.max()))
    return fx


def deployed_fixture(filters: int, flavour: str, seed: int = 0, nframes: int = 64) -> Fixture:
    rng = np.random.default_rng([seed, filters, flavour == "dense", 1])
    tap = 4 if flavour == "dense" else 1                 # dense: conv outputs up to 3 * 8 + 2 = 26 units (e4m3 rounds them)
    ck = rng.integers(1, tap + 1, size=(1, 2, 1, filters)) * rng.choice([-1.0, 1.0], size=(1, 2, 1, filters))
    cb = _signs(rng, filters, [1.0, 2.0]) * U
    if flavour == "dense":      # filters 0 / 1: 4 (x[w-1] + x[w]) +- 1 units -- 17, 21, 25 are e4m3 ties that round DOWN to even, 19, 23 ties that round UP
        ck[..., 0], cb[0] = 4.0, U
        ck[..., 1], cb[1] = 4.0, -U
    dk = rng.integers(-2, 3, size=(258 * filters, 3)).astype(np.float64)
    db = _signs(rng, 3, [8.0, 16.0, 24.0]) * U
    x = fixture_frames(nframes, seed + 2, amp=3)
    ref = O.forward_deployed(x, ck, cb, dk, db, dtype=np.float64)
    s = _spread_dense2(float(np.abs(ref["dense"]).max()))
    dk, db = dk * s, db * s
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    fx = Fixture("deployed", (filters, 3), flavour, [(f32(ck), f32(cb)), (f32(dk), f32(db))], x)
    fx.fp8_input_absmax = _pow2_at_least(float(np.abs(x).max()))
    return fx


def cnnpy_frames(n: int, seed: int) -> np.ndarray:
    return fixture_frames(n, seed, amp=3)


def cnnpy_fixture(shape: Tuple[int, int, int], flavour: str, seed: int = 0, nframes: int = 64) -> Fixture:
    F, D, C = shape
    rng = np.random.default_rng([seed, F, D, C, flavour == "dense", 2])
    ck = _ternary(rng, (1, 2, 128, F), 0.75 if flavour == "dense" else 0.05)
    ck[0, 0, 0, :] = 1.0                                  # no all-zero filter
    cb = _signs(rng, F, [1.0, 2.0, 3.0]) * U
    k1 = rng.integers(-2, 3, size=(3 * F, D)).astype(np.float64)
    k1[0, :] = 1.0
    b1 = _signs(rng, D, [1.0, 2.0, 3.0]) * U
    x = cnnpy_frames(nframes, seed + 3)
    hid = O.dense(O.cnnpy_conv(x, ck, cb, np.float64).reshape(nframes, -1), k1, b1, True, np.float64)

    def draw(r):
        k = r.integers(-2, 3, size=(D, C)).astype(np.float64)
        k[0, :] = np.where(k[0, :] == 0, 1.0, k[0, :])
        return k
    k2, b2, pair, lg = _draw_head(hid, C, [seed, F, D, C, flavour == "dense"], draw)
    s = _spread_dense2(float(np.abs(lg).max()))
    k2, b2 = k2 * s, b2 * s
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    return Fixture("cnnpy", shape, flavour, [(f32(ck), f32(cb)), (f32(k1), f32(b1)), (f32(k2), f32(b2))], x, pair)


# ----------------------------------------------------------------------------------------------------------------------
# the library's power-of-two scales, as its packers choose them (restated here because the preconditions depend on them)
# ----------------------------------------------------------------------------------------------------------------------
def _floor_log2_224_over(v: float) -> int:
    return int(np.floor(np.log2(np.float32(224.0) / np.float32(v))))


def fp8_scales(fx: Fixture) -> Dict[str, int]:
    """log2 of the e4m3 scales: activations 2^sa, weights 2^sw, VT-CNN2 features 2^kf."""
    if fx.kind == "vtcnn2":
        (k1, b1), (k2, _), _, _ = fx.weights
        bound = (fx.fp8_input_absmax * np.abs(k1.reshape(256, 3)).sum(axis=1) + np.abs(b1)).max()     # vtcnn2_fp8_conv.hip:469-475
        return {"sa": _floor_log2_224_over(bound), "sw": _floor_log2_224_over(np.abs(k2).max()),      # :474
                "kf": _floor_log2_224_over(fx.fp8_feature_absmax)}                                    # :548
    (ck, cb), (dk, _) = fx.weights
    k = ck.reshape(2, -1)
    bound = (fx.fp8_input_absmax * (np.abs(k[0]) + np.abs(k[1])) + np.abs(cb)).max()                 # deployed_bf16.hip:527
    return {"sa": _floor_log2_224_over(bound), "sw": _floor_log2_224_over(np.abs(dk).max())}         # :530


# ----------------------------------------------------------------------------------------------------------------------
# quantisation-aware oracle
# ----------------------------------------------------------------------------------------------------------------------
class _Trace:
    """What `expected()` saw at each narrowing point and accumulation, for the precondition checker and the CPU tests."""

    def __init__(self, corrupt=None):
        self.points: List[Tuple[str, str, int, np.ndarray, np.ndarray]] = []      # (name, type, log2 scale, before, after)
        self.sums: List[Tuple[str, tuple]] = []                                    # (name, (layer fn, input, kernel, bias))
        self.corrupt = corrupt

    def narrow(self, name: str, typ: Optional[str], a, scale_log2: int = 0, second: Optional[str] = None):
        """a -> typ(a 2^scale) 2^-scale.  `second`: the type of a second conversion applied to the first one's result."""
        a = np.asarray(a, np.float64)
        if typ is None:
            return a
        trunc = self.corrupt == ("trunc", name)
        v = np.ldexp(a, scale_log2)
        r = NARROW[typ](v, trunc=trunc)
        self.points.append((name, typ, scale_log2, v, r))
        if second is not None:
            r2 = NARROW[second](r)
            self.points.append((name + "/2", second, scale_log2, r, r2))
            r = r2
        return np.ldexp(r, -scale_log2)

    def layer(self, name, fn, x, k, b, *args):
        self.sums.append((name, (fn, x, k, b, args)))
        if self.corrupt == ("bias", name):
            b = np.array(b, np.float64)
            b[0] = 0.0
        return fn(x, k, b, *args, dtype=np.float64)

    def swap(self, name, feat, i0, i1):
        """The 'swap' fault: the feature positions i0 and i1 (index tuples after the frame axis) exchange places in every frame."""
        if self.corrupt != ("swap", name):
            return feat
        f = np.array(feat)
        s0, s1 = (slice(None),) + i0, (slice(None),) + i1
        f[s0], f[s1] = feat[s1], feat[s0]
        return f


def expected(fx: Fixture, mode: str = "f32", fp8_bf16_features: bool = False, corrupt=None, frames=None):
    """The arrays the GPU must return on this fixture in this mode, as f64, and the trace of how they came about.
    corrupt: None, or ('swap' | 'bias' | 'trunc', point / layer name) -- the sensitivity check's faults."""
    t = _Trace(corrupt)
    x = fx.frames if frames is None else frames
    w = [np.asarray(a, np.float64) for a in fx.flat_weights]
    if fx.kind == "vtcnn2":
        k1, b1, k2, b2, w1, c1, w2, c2 = w
        low = mode != "f32"
        sc = fp8_scales(fx) if mode == "fp8" else {"sa": 0, "sw": 0, "kf": 0}
        e4feat = mode == "fp8" and not fp8_bf16_features
        xq = t.narrow("frames", "bf16x2" if low else None, x)
        k1q = t.narrow("conv1.taps", "bf16x2" if low else None, k1)
        b1q = t.narrow("conv1.bias", "bf16x2" if low else None, b1)
        y1 = t.layer("conv1", O.vtcnn2_conv1, xq, k1q, b1q)
        if mode == "fp8":
            y1 = t.narrow("conv1.out", "bf16", y1, sc["sa"], second="e4m3")
            k2q = t.narrow("conv2.weights", "e4m3", k2, sc["sw"])
        else:
            y1 = t.narrow("conv1.out", "bf16" if low else None, y1)
            k2q = t.narrow("conv2.weights", "bf16" if low else None, k2)
        y2 = t.layer("conv2", O.vtcnn2_conv2, y1, k2q, b2)
        y2 = t.narrow("conv2.out", "e4m3" if e4feat else ("bf16" if low else None), y2, sc["kf"] if e4feat else 0)
        y2 = t.swap("conv2", y2, (0, 5), (0, 6))             # channel 0, positions 5 and 6
        flat = y2.reshape(y2.shape[0], -1)
        w1q = t.narrow("dense1.weights", "bf16" if low else None, w1)
        hid = t.layer("dense1", O.dense, flat, w1q, c1, True)
        lg = t.layer("dense2", O.dense, hid, w2, c2, False)
        out = {"conv": y2, "flat": flat, "hidden": hid, "dense": lg}
    elif fx.kind == "deployed":
        ck, cb, dk, db = w
        sc = fp8_scales(fx) if mode == "fp8" else {"sa": 0, "sw": 0}
        h = "f16" if mode == "f16" else None
        xq, ckq, cbq = t.narrow("frames", h, x), t.narrow("conv.taps", h, ck), t.narrow("conv.bias", h, cb)
        y = t.layer("conv", O.deployed_conv, xq, ckq, cbq)
        typ = {"f32": None, "bf16": "bf16", "f16": "f16", "fp8": "e4m3"}[mode]
        y = t.narrow("conv.out", typ, y, sc["sa"])
        y = t.swap("conv", y, (0, 5, 0), (0, 6, 0))           # row 0, positions 5 and 6, filter 0
        flat = y.reshape(y.shape[0], -1)
        dkq = t.narrow("dense.weights", typ, dk, sc["sw"])
        d = t.layer("dense", O.dense, flat, dkq, db, True)
        out = {"conv": y, "flat": flat, "dense": d}
        lg = d
    else:
        ck, cb, k1, b1, k2, b2 = w
        assert mode == "f32", "cnn.py's net runs at f32 only"
        y = t.layer("conv", O.cnnpy_conv, x, ck, cb)
        y = t.swap("conv", y, (0, 0), (1, 0))                 # positions 0 and 1, filter 0
        flat = y.reshape(y.shape[0], -1)
        hid = t.layer("dense1", O.dense, flat, k1, b1, True)
        lg = t.layer("dense2", O.dense, hid, k2, b2, False)
        out = {"conv": y.reshape(-1, 1, 3, fx.shape[0]), "flat": flat, "hidden": hid, "dense": lg}
    out["probs"] = O.softmax(lg)
    out["labels"] = O.argmax_first(lg)
    return out, t


def plain(fx: Fixture, frames=None) -> Dict[str, np.ndarray]:
    """The plain f64 oracle on the fixture (whole-net forward of oracle_np)."""
    return O.forward(fx.kind, fx.frames if frames is None else frames, fx.weights, dtype=np.float64)


# ----------------------------------------------------------------------------------------------------------------------
# preconditions
# ----------------------------------------------------------------------------------------------------------------------
def _lsb_log2(a) -> int:
    """log2 of the largest power of two that divides every non-zero element of `a` (a large value if there is none)."""
    a = np.abs(np.asarray(a, np.float64)).ravel()
    a = a[a != 0]
    if a.size == 0:
        return 1 << 20
    m, e = np.frexp(a)
    M = np.ldexp(m, 53).astype(np.int64)
    low = (M & -M).astype(np.float64)
    return int((e - 53 + np.log2(low).astype(np.int64)).min())


def check_preconditions(fx: Fixture, mode: str = "f32", fp8_bf16_features: bool = False, verbose: bool = False, frames=None) -> Dict[str, float]:
    """Asserts, on the oracle alone, that the GPU must reproduce `expected()` bit for bit, and returns the bounds it found.
    frames: other frames than the fixture's own (the same preconditions, checked on them)."""
    return _check(fx, mode, fp8_bf16_features, verbose, frames)[0]


def checked_expected(fx: Fixture, mode: str = "f32", fp8_bf16_features: bool = False, frames=None) -> Dict[str, np.ndarray]:
    """`expected()`'s arrays, handed out only after the preconditions held on them (one oracle pass for both)."""
    return _check(fx, mode, fp8_bf16_features, False, frames)[1]


def _check(fx: Fixture, mode: str, fp8_bf16_features: bool, verbose: bool, frames):
    out, t = expected(fx, mode, fp8_bf16_features, frames=frames)
    tag = f"{fx.kind}{fx.shape} {fx.flavour} {mode}{'+bf16feat' if fp8_bf16_features else ''}"
    bounds: Dict[str, float] = {}
    # 1. every accumulation: sum |term| in units of the smallest bit any term can carry, below 2^24
    for name, (fn, x, k, b, args) in t.sums:
        unit = min(_lsb_log2(x) + _lsb_log2(k), _lsb_log2(b))
        s = fn(np.abs(x), np.abs(k), np.abs(b), *args, dtype=np.float64)      # all terms positive: the ReLU is the identity
        units = float(np.ldexp(np.abs(s).max(), -unit))
        assert units < EXACT_F32, f"{tag}: {name}: sum |term| = {units:.3g} units (unit 2^{unit}) is not below 2^24"
        if mode == "f16" and name == "conv":      # the f16 mode's conv is two packed-f16 fmas: its partial sums must be f16 integers
            assert units < 2048, f"{tag}: conv: {units} units do not fit f16's 11 bits"
        bounds[f"{name} sum|term| (units)"] = units
    # 2. every narrowing point: the value fits the type, or is an integer of at most 255 units rounded ONCE; range
    for name, typ, sl, before, after in t.points:
        nz = np.abs(before[before != 0])
        fits = after == before
        integer = (before == np.rint(before)) & (np.abs(before) <= 255)
        assert (fits | integer).all(), f"{tag}: {name}: a value neither fits {typ} nor is an integer <= 255 at scale 2^{sl}"
        if name.endswith("/2"):     # second conversion of a two-step one: its input must be what the first step was given
            first = [p for p in t.points if p[0] == name[:-2]][0]
            assert (first[4] == first[3]).all(), f"{tag}: {name}: the first step already rounded: two roundings"
        if nz.size:
            assert nz.min() >= _MIN_NORMAL[typ], f"{tag}: {name}: {nz.min():.3g} is subnormal in {typ} at scale 2^{sl}"
            assert nz.max() <= _MAX_FINITE[typ], f"{tag}: {name}: {nz.max():.3g} saturates {typ} at scale 2^{sl}"
        bounds[f"{name} -> {typ} max (scaled)"] = float(nz.max()) if nz.size else 0.0
        bounds[f"{name} -> {typ} rounded"] = float((~fits).mean())
    # 3. the asserted arrays themselves are f32 numbers
    for key in ("conv", "flat", "hidden", "dense"):
        if key in out:
            assert (out[key].astype(np.float32).astype(np.float64) == out[key]).all(), f"{tag}: expected '{key}' is not exact in f32"
    # 4. fixture content: biases of both signs in every layer; ties; labels
    for i, (_k, b) in enumerate(fx.weights):
        assert (b != 0).all() and ((b > 0).any() and (b < 0).any() or b.size == 1), f"{tag}: layer {i}: biases must be non-zero, of both signs"
    lg = out["dense"]
    if fx.tie_pair is not None:
        i, j = fx.tie_pair
        assert (lg[:, i] == lg[:, j]).all()
        top = (lg[:, i] == lg.max(axis=1))
        assert top.any(), f"{tag}: the tied pair is the maximum on no frame"
        assert (out["labels"][top] <= min(i, j)).all()                            # the oracle itself lets the first index win
        bounds["frames whose maximum is the tied pair"] = float(top.sum())
    if fx.kind == "vtcnn2" and fx.shape[0] >= 11:
        assert len(np.unique(out["labels"])) >= 4, f"{tag}: labels take only {np.unique(out['labels'])}"
    bounds["distinct labels"] = float(len(np.unique(out["labels"])))
    bounds["max |logit|"] = float(np.abs(lg).max())
    # 5. fp8 on the dense flavour: the rounding is real and includes round-to-even ties
    if mode == "fp8" and fx.flavour == "dense" and not fp8_bf16_features:
        name = "conv2.out" if fx.kind == "vtcnn2" else "conv.out"
        p = [q for q in t.points if q[0] == name][0]
        ties = is_e4m3_tie(p[3])
        assert ties.any(), f"{tag}: no feature is a round-to-even tie"
        bounds[f"{name} e4m3 ties"] = float(ties.mean())
    if verbose:
        print(f"[exact fixture] {tag}")
        for k, v in bounds.items():
            print(f"    {k}: {v:.6g}")
    return bounds, out


def batch_indices(n: int, nframes: int, seed: int) -> np.ndarray:
    """A batch of n frames out of the fixture's nframes: every fixture frame at least once if n allows, seeded order."""
    rng = np.random.default_rng([seed, n])
    idx = np.concatenate([np.arange(nframes)] * (n // nframes) + [rng.choice(nframes, size=n % nframes, replace=False)])
    return rng.permutation(idx)


# ----------------------------------------------------------------------------------------------------------------------
# raw uint8 I/Q captures that stand for exact frames
# ----------------------------------------------------------------------------------------------------------------------
# (byte - 127.5) 2^-6 = (2 byte - 255) U: an odd number of units, exact in f32 (127.5 and 2^-6 are f32 numbers, the difference
# has at most 9 significant bits).  Bytes 127 / 128 are +-U, VT-CNN2's amp = 1 range without its zeros; bytes 126..129 are +-U
# and +-3U, the deployed nets' amp = 3 range.  The fixtures' weights, scales and fp8_input_absmax = U serve unchanged.
RAW_SCALE = 2.0 ** -6
RAW_BYTES = {"vtcnn2": (127, 128), "deployed": (126, 127, 128, 129)}
RAW_FRAMES = 64                                   # raw fixture frames of the hop-128 layout, as many as Fixture.frames
RAW_PERIOD = {64: 64 * 128, 3: 384}               # pairs per period of the periodic layouts: 128 distinct windows each


def raw_fixture_frames(kind: str, seed: int) -> np.ndarray:
    """The RAW_FRAMES raw fixture frames: (64, 256) uint8, 128 (I, Q) byte pairs each, seeded draws from RAW_BYTES[kind]."""
    rng = np.random.default_rng([seed, len(RAW_BYTES[kind]), 128])
    return rng.choice(np.array(RAW_BYTES[kind], np.uint8), size=(RAW_FRAMES, 256))


def raw_capture(kind: str, hop: int, seed: int, idx=None, windows: Optional[int] = None) -> np.ndarray:
    """The uint8 stream I0, Q0, I1, Q1, ... of a capture whose windows (128 pairs, `hop` pairs apart) are exact fixture frames.
    hop 128: window i is raw fixture frame idx[i] (idx from batch_indices); the oracle runs on the 64 raw frames
             (idx = arange(RAW_FRAMES)) and the expectation is want[idx].
    hop 64, 3: `windows` windows of a periodic stream, period RAW_PERIOD[hop] pairs = 128 hops: window i is window i mod 128;
             the oracle runs on raw_capture(..., windows=128) and the expectation is want[arange(windows) % 128]."""
    if hop == 128:
        assert idx is not None and windows is None
        return np.ascontiguousarray(raw_fixture_frames(kind, seed)[np.asarray(idx)]).reshape(-1)
    assert idx is None and windows is not None and windows >= 1
    period = RAW_PERIOD[hop]
    assert period % hop == 0
    rng = np.random.default_rng([seed, len(RAW_BYTES[kind]), hop])
    one = rng.choice(np.array(RAW_BYTES[kind], np.uint8), size=2 * period)
    pairs = (windows - 1) * hop + 128
    return np.ascontiguousarray(np.tile(one, -(-pairs // period))[:2 * pairs])


def raw_period_windows(hop: int) -> int:
    """Distinct windows of the periodic layout at this hop."""
    return RAW_PERIOD[hop] // hop


def raw_windows(stream, hop: int, scale: float = RAW_SCALE, first_pair: int = 0, swap_iq: bool = False) -> np.ndarray:
    """The library's windowing and conversion (mdc_iq_u8_windows, include/mdc.h) restated in numpy f32: window i is pairs
    [i hop, i hop + 128), row 0 = (I - 127.5) scale from the even bytes, row 1 = (Q - 127.5) scale from the odd ones.
    first_pair / swap_iq: the sensitivity check's faults (window i taken from pair i hop + first_pair; I and Q exchanged)."""
    pairs = np.asarray(stream, np.uint8).reshape(-1, 2)
    n = 0 if len(pairs) < 128 + first_pair else (len(pairs) - 128 - first_pair) // hop + 1
    at = np.arange(n)[:, None] * hop + first_pair + np.arange(128)[None, :]
    w = pairs[at].astype(np.float32)                       # (n, 128, 2)
    if swap_iq:
        w = w[:, :, ::-1]
    sc = np.float32(scale)
    return np.ascontiguousarray(np.stack([(w[:, :, 0] - np.float32(127.5)) * sc, (w[:, :, 1] - np.float32(127.5)) * sc], axis=1))


def raw_oracle_frames(kind: str, hop: int, seed: int) -> np.ndarray:
    """The distinct windows of a layout, as frames: what the oracle is run on (64 at hop 128, 128 at the periodic hops)."""
    if hop == 128:
        return raw_windows(raw_capture(kind, 128, seed, idx=np.arange(RAW_FRAMES)), 128)
    return raw_windows(raw_capture(kind, hop, seed, windows=raw_period_windows(hop)), hop)
