"""CPU side of the exact-integer fixtures (tests/exact_fixtures.py): the preconditions hold for every fixture, flavour and
mode; the narrowing functions are torch's casts; the quantisation-aware oracle is the plain f64 oracle wherever no
narrowing rounds; and the faults the fixtures exist for -- two feature positions swapped, one channel's bias dropped, one
conversion truncating -- each change an array the GPU tests assert (tests/test_exact_fixtures_gpu.py)."""
import numpy as np
import pytest
import torch

import exact_fixtures as X

VT = [(c, f) for c in (11, 16) for f in ("dense", "sparse")]
DEP = [(F, f) for F in (3, 10) for f in ("dense", "sparse")]
CNNPY = [(s, f) for s in ((10, 16, 16), (1, 1, 1), (10, 10, 5)) for f in ("dense", "sparse")]
_cache = {}


def _fx(kind, shape, flavour):
    key = (kind, shape, flavour)
    if key not in _cache:
        _cache[key] = {"vtcnn2": lambda: X.vtcnn2_fixture(shape, flavour), "deployed": lambda: X.deployed_fixture(shape, flavour),
                       "cnnpy": lambda: X.cnnpy_fixture(shape, flavour)}[kind]()
    return _cache[key]


def _all_cases():
    for c, f in VT:
        for mode, bf in X.VT_MODES:
            yield "vtcnn2", c, f, mode, bf
    for F, f in DEP:
        for mode in X.DEP_MODES:
            yield "deployed", F, f, mode, False
    for s, f in CNNPY:
        yield "cnnpy", s, f, "f32", False


CASES = list(_all_cases())
IDS = [f"{k}-{s}-{f}-{m}{'-bf16feat' if b else ''}" for k, s, f, m, b in CASES]


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape,flavour,mode,bf", CASES, ids=IDS)
def test_preconditions_hold(kind, shape, flavour, mode, bf):
    bounds = X.check_preconditions(_fx(kind, shape, flavour), mode, bf, verbose=True)      # (prints its bounds: pytest -s)
    assert all(v < X.EXACT_F32 for k, v in bounds.items() if "sum|term|" in k)
    fx = _fx(kind, shape, flavour)
    if kind == "vtcnn2":                      # the frames the issue names
        x = fx.frames
        assert not x[0].any()
        for i, (h, s) in enumerate([(0, 0), (0, 127), (1, 0), (1, 127), (0, 63)], start=1):
            assert np.count_nonzero(x[i]) == 1 and x[i, h, s] != 0
        assert len(x) <= 64


def test_preconditions_reject_a_fixture_that_breaks_them():
    """The checker is an assertion, not a filter: a fixture whose features no longer fit e4m3 as single-rounded integers, whose
    sums leave f32's integers, or whose activations go subnormal is an error."""
    fx = _fx("vtcnn2", 11, "dense")
    bad = X.Fixture(**{**fx.__dict__, "fp8_feature_absmax": fx.fp8_feature_absmax * 8})        # features x 2^-3: no longer integers
    with pytest.raises(AssertionError):
        X.check_preconditions(bad, "fp8")
    w = [(k.copy(), b.copy()) for k, b in fx.weights]
    w[2] = (w[2][0] * np.float32(1025.0), w[2][1])                                          # dense1 sums beyond 2^24 units
    with pytest.raises(AssertionError):
        X.check_preconditions(X.Fixture(**{**fx.__dict__, "weights": w}), "f32")
    with pytest.raises(AssertionError):                                                     # stated range 2^13 too wide: subnormal e4m3
        X.check_preconditions(X.Fixture(**{**fx.__dict__, "fp8_input_absmax": fx.fp8_input_absmax * 2.0 ** 13}), "fp8")


# ---------------------------------------------------------------------------------------------------------------
# narrowing functions against torch's CPU casts
# ---------------------------------------------------------------------------------------------------------------
def _torch_cast(v, dtype):
    return torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(dtype).to(torch.float32).numpy().astype(np.float64)


def _e4m3_table():
    """All 256 OCP e4m3fn codes, literally: sign, 4 exponent bits (bias 7), 3 mantissa bits; 0x7F / 0xFF are NaN."""
    vals = []
    for c in range(256):
        s, e, m = c >> 7, (c >> 3) & 15, c & 7
        v = np.nan if (e == 15 and m == 7) else ((m / 8) * 2.0 ** -6 if e == 0 else (1 + m / 8) * 2.0 ** (e - 7))
        vals.append(-v if s else v)
    return np.array(vals)


def _sweep():
    """Ties and their neighbours on every binade the types share, and the ends of the e4m3 / f16 ranges."""
    t = _e4m3_table()
    pos = np.sort(t[np.isfinite(t) & (t > 0)])
    mid = (pos[:-1] + pos[1:]) / 2                                             # every e4m3 tie
    near = np.concatenate([np.nextafter(mid.astype(np.float32), np.float32(0)), np.nextafter(mid.astype(np.float32), np.float32(1e9))]).astype(np.float64)
    k = np.arange(0, 1 << 12, dtype=np.float64)                                # 12-bit integers: every bf16 and f16 tie pattern
    ints = np.concatenate([k * 2.0 ** e for e in (-20, -7, 0, 4)])
    ends = np.array([0.0, 2.0 ** -9, 2.0 ** -10, 3 * 2.0 ** -11, 2.0 ** -6, 440.0, 447.9, 448.0, 2.0 ** -14, 2.0 ** -24, 65504.0, 65519.0])
    v = np.concatenate([pos, mid, near, ints, ends])
    return np.concatenate([v, -v])


def test_narrowing_functions_are_torch_casts_on_a_sweep_of_ties_and_range_ends():
    v = _sweep()
    assert np.array_equal(X.narrow_bf16(v), _torch_cast(v, torch.bfloat16))
    h = v[np.abs(v) < 65520.0]                                                 # beyond: inf in torch, never reached by a fixture
    assert np.array_equal(X.narrow_f16(h), _torch_cast(h, torch.float16))
    e = v[np.abs(v) <= 448.0]                                                  # beyond: the kernels saturate, torch gives NaN
    assert np.array_equal(X.narrow_e4m3(e), _torch_cast(e, torch.float8_e4m3fn))
    table = _e4m3_table()
    fin = table[np.isfinite(table)]
    assert np.array_equal(X.narrow_e4m3(fin), fin) and len(np.unique(fin)) == 253      # the codes are fixed points (+-0 are one value)
    assert np.array_equal(X.narrow_e4m3(np.array([449.0, 1e6, -1e6])), [448.0, 448.0, -448.0])
    assert X.is_e4m3_tie(np.array([17.0, 19.0, 68.0, 2.0 ** -9 * 2.5])).all() and not X.is_e4m3_tie(np.array([16.0, 18.0, 17.5, 0.0])).any()
    # truncation (the sensitivity check's fault) never exceeds the value and differs from RNE on the upper half
    assert (np.abs(X.narrow_e4m3(e, trunc=True)) <= np.abs(e)).all() and (X.narrow_e4m3(np.array([19.0]), trunc=True) == 18.0).all()
    assert (np.abs(X.narrow_bf16(v, trunc=True)) <= np.abs(v)).all() and (np.abs(X.narrow_f16(h, trunc=True)) <= np.abs(h)).all()


@pytest.mark.parametrize("kind,shape,flavour,mode,bf", [c for c in CASES if c[3] != "f32"], ids=[i for i, c in zip(IDS, CASES) if c[3] != "f32"])
def test_narrowing_functions_are_torch_casts_on_every_fixture_value(kind, shape, flavour, mode, bf):
    _out, t = X.expected(_fx(kind, shape, flavour), mode, bf)
    cast = {"bf16": torch.bfloat16, "f16": torch.float16, "e4m3": torch.float8_e4m3fn}
    assert t.points
    for name, typ, _sl, before, after in t.points:
        if typ == "bf16x2":
            hi = _torch_cast(before, torch.bfloat16)
            want = hi + _torch_cast(before - hi, torch.bfloat16)
        else:
            want = _torch_cast(before, cast[typ])
        assert np.array_equal(after, want), (name, typ)


# ---------------------------------------------------------------------------------------------------------------
# quantisation-aware oracle against the plain one
# ---------------------------------------------------------------------------------------------------------------
_PLAIN = {"vtcnn2": {"flat": "flat", "hidden": "dense1", "dense": "logits"}, "deployed": {"conv": "conv", "flat": "flat", "dense": "dense"},
          "cnnpy": {"flat": "flat", "hidden": "dense1", "dense": "logits"}}


@pytest.mark.parametrize("kind,shape,flavour,mode,bf", CASES, ids=IDS)
def test_quantisation_aware_oracle_against_the_plain_oracle(kind, shape, flavour, mode, bf):
    """Sparse flavour: equal to the plain f64 oracle, every array, every mode.  Dense flavour: equal up to the first narrowing
    that rounds; there the difference sits exactly on the elements that conversion changed."""
    fx = _fx(kind, shape, flavour)
    out, t = X.expected(fx, mode, bf)
    ref = X.plain(fx)
    rounded = [(name, before != after) for name, _typ, _sl, before, after in t.points if (before != after).any()]
    if flavour == "sparse" or not rounded:
        assert not rounded, [n for n, _ in rounded]
        for key, pk in _PLAIN[kind].items():
            assert np.array_equal(out[key], ref[pk]), key
        assert np.array_equal(out["labels"], ref["labels"]) and np.array_equal(out["probs"], ref["probs"])
        return
    # only the e4m3 features (vtcnn2) / conv outputs (deployed) round, and only in fp8 mode
    assert mode == "fp8" and not bf and [n for n, _ in rounded] == ["conv2.out" if kind == "vtcnn2" else "conv.out"]
    mask = rounded[0][1].reshape(out["flat"].shape)
    assert np.array_equal(out["flat"] != ref["flat"], mask)
    assert not np.array_equal(out["dense"], ref[_PLAIN[kind]["dense"]])              # ... and the rounding reaches the logits


# ---------------------------------------------------------------------------------------------------------------
# sensitivity: the faults these fixtures exist for change an asserted array
# ---------------------------------------------------------------------------------------------------------------
def _asserted(kind, mode):
    if kind == "deployed" and mode != "f32":
        return ()                                  # the reduced modes of the deployed nets have no taps: probabilities and labels only
    return {"vtcnn2": ("flat", "conv", "hidden", "dense"), "deployed": ("dense", "conv"), "cnnpy": ("conv", "hidden", "dense")}[kind]


def _detected(kind, mode, good, bad):
    if any(not np.array_equal(good[k], bad[k]) for k in _asserted(kind, mode)):
        return True
    # probabilities are held to 2e-6: a fault counts as seen only if it moves one by ten times that, or a label
    return bool(np.abs(good["probs"] - bad["probs"]).max() > 2e-5 or not np.array_equal(good["labels"], bad["labels"]))


@pytest.mark.parametrize("kind,shape,flavour,mode,bf", CASES, ids=IDS)
def test_sensitivity_to_a_swap_and_to_a_dropped_bias(kind, shape, flavour, mode, bf):
    fx = _fx(kind, shape, flavour)
    good = X.expected(fx, mode, bf)[0]
    conv = "conv2" if kind == "vtcnn2" else "conv"
    for fault in (("swap", conv), ("bias", conv)):
        assert _detected(kind, mode, good, X.expected(fx, mode, bf, corrupt=fault)[0]), fault


@pytest.mark.parametrize("kind,shape,mode", [("vtcnn2", 11, "fp8"), ("vtcnn2", 16, "fp8"), ("deployed", 3, "fp8"), ("deployed", 10, "fp8")])
def test_sensitivity_to_a_truncating_conversion(kind, shape, mode):
    """Truncation instead of round-to-even at the one narrowing point that rounds (the dense flavour's e4m3 features).  cnn.py's
    net has no narrowing point, and in the other modes every conversion is the identity on these fixtures: nothing to truncate."""
    fx = _fx(kind, shape, "dense")
    good = X.expected(fx, mode)[0]
    point = "conv2.out" if kind == "vtcnn2" else "conv.out"
    assert _detected(kind, mode, good, X.expected(fx, mode, corrupt=("trunc", point))[0])


# ---------------------------------------------------------------------------------------------------------------
# raw uint8 I/Q captures (exact_fixtures.raw_capture / raw_windows): the byte streams tests/test_exact_walks_gpu.py feeds to
# predict_iq_u8 stand for exact frames, the preconditions hold on them, and a window taken one pair off changes the expectation
# ---------------------------------------------------------------------------------------------------------------
RAW_SEED = 0            # (the GPU file's seed; the preconditions below are what qualifies it)
RAW_HOPS = (128, 64, 3)
RAW_CASES = [c for c in CASES if c[0] != "cnnpy"]      # cnn.py's net converts first and forwards frames: no raw-byte kernel
RAW_IDS = [i for i, c in zip(IDS, CASES) if c[0] != "cnnpy"]


@pytest.mark.parametrize("kind", ["vtcnn2", "deployed"])
def test_raw_captures_stand_for_odd_multiples_of_the_unit(kind):
    units = {"vtcnn2": {-1, 1}, "deployed": {-3, -1, 1, 3}}[kind]
    raw = X.raw_fixture_frames(kind, RAW_SEED)
    assert raw.shape == (64, 256) and raw.dtype == np.uint8 and set(np.unique(raw)) == set(X.RAW_BYTES[kind])
    # hop 128: window i is raw fixture frame idx[i]: I from the even bytes, Q from the odd ones, (2 byte - 255) U exactly
    idx = X.batch_indices(257, 64, seed=257)
    stream = X.raw_capture(kind, 128, RAW_SEED, idx=idx)
    assert stream.dtype == np.uint8 and stream.shape == (257 * 256,)
    fr = X.raw_windows(stream, 128)
    assert fr.dtype == np.float32 and fr.shape == (257, 2, 128)
    want = (2 * raw[idx].astype(np.int64).reshape(257, 128, 2).transpose(0, 2, 1) - 255) * X.U      # integers times 2^-7: exact in f64
    assert np.array_equal(fr.astype(np.float64), want)
    assert set(np.unique(fr.astype(np.float64) / X.U)) == units
    assert np.array_equal(X.raw_oracle_frames(kind, 128, RAW_SEED)[idx], fr)
    # the periodic layouts: 128 distinct windows, window i = window i mod 128, however long the stream is
    for hop in (64, 3):
        assert X.raw_period_windows(hop) == 128
        n = 128 * 2 + 37
        stream = X.raw_capture(kind, hop, RAW_SEED, windows=n)
        assert stream.shape == (2 * ((n - 1) * hop + 128),)
        fr = X.raw_windows(stream, hop)
        one = X.raw_oracle_frames(kind, hop, RAW_SEED)
        assert fr.shape == (n, 2, 128) and one.shape == (128, 2, 128)
        assert np.array_equal(fr, one[np.arange(n) % 128])
        assert set(np.unique(fr.astype(np.float64) / X.U)) == units
        assert len(np.unique(one.reshape(128, -1), axis=0)) == 128                # ... and they ARE distinct
        pairs = stream.reshape(-1, 2)
        assert np.array_equal(fr[5, 0], (2.0 * pairs[5 * hop:5 * hop + 128, 0] - 255) * X.U)      # I: even bytes, from pair i hop
        assert np.array_equal(fr[5, 1], (2.0 * pairs[5 * hop:5 * hop + 128, 1] - 255) * X.U)


@pytest.mark.parametrize("kind,shape,flavour,mode,bf", RAW_CASES, ids=RAW_IDS)
def test_preconditions_hold_on_the_raw_byte_frames(kind, shape, flavour, mode, bf):
    """The fixtures' weights, scales and fp8_input_absmax = U serve the raw-byte frames unchanged, at every hop (prints the
    bounds: pytest -s).  A failure is an error of the fixture, as above."""
    fx = _fx(kind, shape, flavour)
    for hop in RAW_HOPS:
        fr = X.raw_oracle_frames(kind, hop, RAW_SEED)
        assert float(np.abs(fr).max()) <= fx.fp8_input_absmax                     # the range the fp8 mode was told to represent
        bounds = X.check_preconditions(fx, mode, bf, verbose=True, frames=fr)
        assert all(v < X.EXACT_F32 for k, v in bounds.items() if "sum|term|" in k)
        if kind == "vtcnn2":
            assert bounds["distinct labels"] >= 4 and bounds["frames whose maximum is the tied pair"] >= 1


def _raw_faults(kind, hop):
    """(name, frames) of the three faults on the first 16 windows of a capture (the oracle's cost is per window; a fault that
    moves every window shows on 16), cut from a stream a few windows longer so that every faulty window exists."""
    n = 16
    stream = X.raw_capture(kind, 128, RAW_SEED, idx=np.arange(n + 1) % 64) if hop == 128 else X.raw_capture(kind, hop, RAW_SEED, windows=n + 128 // hop + 1)
    good = X.raw_windows(stream, hop)[:n]
    yield "good", good
    yield "stream shifted by one pair", X.raw_windows(stream[2:], hop)[:n]
    yield "I and Q exchanged", X.raw_windows(stream, hop, swap_iq=True)[:n]
    yield "window i from pair i hop + 1", X.raw_windows(stream, hop, first_pair=1)[:n]


@pytest.mark.parametrize("hop", RAW_HOPS)
@pytest.mark.parametrize("kind,shape,flavour,mode,bf", [c for c in RAW_CASES if c[1] in (11, 3, 10)], ids=[i for i, c in zip(RAW_IDS, RAW_CASES) if c[1] in (11, 3, 10)])
def test_sensitivity_of_the_raw_byte_expectation(kind, shape, flavour, mode, bf, hop):
    """A capture read one pair late, with I and Q exchanged, or with each window taken from pair i hop + 1 changes the expected
    `dense` array, and with it an array the GPU tests assert (the deployed nets' reduced modes: probabilities and labels only)."""
    fx = _fx(kind, shape, flavour)
    runs = {name: X.expected(fx, mode, bf, frames=fr)[0] for name, fr in _raw_faults(kind, hop)}
    good = runs.pop("good")
    for name, bad in runs.items():
        assert not np.array_equal(good["dense"], bad["dense"]), name
        assert (good["dense"] != bad["dense"]).any(axis=1).mean() > 0.5, name          # not one lucky window: most of them
        assert _detected(kind, mode, good, bad), name
