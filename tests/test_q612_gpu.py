"""mdc_forward_q612 (csrc/deployed_q612.hip) on the MI355X against the integer oracle (oracle/oracle_q612.py, numpy int64) where
the kernel can go wrong.  Its contract is that every output word equals the oracle's, so every comparison is assert_array_equal
(or torch.equal between two GPU runs); both `dense` (int32) and `labels` are compared, for F = 3 and F = 10:

  a. full-range 18-bit weights and input words at every ragged block size around 64 and at sizes that fill all four waves of a
     work-group (the F = 10 kernel keeps one LDS weight region per wave) and several work-groups; the same words with random bits
     above bit 17; outputs pre-filled with a sentinel, one guard row / element after them untouched;
  b. one-hot frames (+1.0 or -32.0 at columns 0, 1, 2, 63, 64, 125, 126, 127 of each row): the position-0 tail, lane 63's right
     pad and the lane tables' 2 lane + 1 + s indexing, in a block shared with random frames;
  c. the float quantiser on magnitudes from 2^-14 to just under 2^19 and at its exact edges (include/mdc.h: |v| < 2^19);
  d. frames outside that domain (NaN, Inf, 1e30, 2^19) never change another frame's results;
  e. one batch past the grid cap (Q612_GRID_CAP x 4 waves x Q612_BLOCK_FRAMES frames): the persistent walk's second pass;
  f. first-maximum ties between equal positive sums, and the all-zero tie;
  g. ABI corners: dense_dev / labels_dev NULL, a side stream, the refusal of F = 5.

The weights of (a) to (f) are integers drawn uniformly from [-2^17, 2^17) and handed over as k / 4096 (exact in f32), with one
weight at 40.0 (outside Q6.12: the library and the oracle both wrap it to -24.0).  That such operands exercise both sides of every
ReLU and every label is asserted on the reference (`_assert_mix`)."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from conftest import load_deployed_npz                                                   # noqa: E402
from oracle import oracle_q612 as Q                                                      # noqa: E402
from modulationdetectioncnn_amd import VTCNN2, Topology, _cabi                           # noqa: E402

LO, HI = -(1 << 17), 1 << 17            # the 18-bit range [LO, HI)
SENTINEL = -0x5A5A5A5B                  # negative: no post-ReLU sum and no label can equal it
TRAINED = {3: "3convmodrecnets_CNN2_0.5", 10: "convmodrecnets_CNN2_0.5"}
SEED = {3: 0, 10: 0}                    # seeds of the full-range weights and of the reference batch (conditions: _assert_mix)
ENOTSUP = -95                           # include/mdc.h: MDC_ENOTSUP


# ---------------------------------------------------------------------------------------------------------------- operands and reference
def _full_range_weights(F, seed, rng=None):
    """[(conv kernel (1,2,1,F), bias F), (dense kernel (258F,3), bias 3)] f32 = k / 4096 with k uniform over the 18-bit range, each
    tensor a fresh draw; dense kernel [7, 1] = 40.0, which is not a Q6.12 value: host and oracle wrap it to -24.0."""
    rng = np.random.default_rng(seed) if rng is None else rng
    ck = rng.integers(LO, HI, (1, 2, 1, F)) / 4096.0
    cb = rng.integers(LO, HI, (F,)) / 4096.0
    dk = rng.integers(LO, HI, (258 * F, 3)) / 4096.0
    db = rng.integers(LO, HI, (3,)) / 4096.0
    dk[7, 1] = 40.0
    w = [(ck.astype(np.float32), cb.astype(np.float32)), (dk.astype(np.float32), db.astype(np.float32))]
    for (k32, b32), (k64, b64) in zip(w, [(ck, cb), (dk, db)]):
        assert (k32 == k64).all() and (b32 == b64).all()                 # exact in f32
    assert Q.quantize(w[1][0])[7, 1] == -24 * 4096
    return w


def _words(rng, n):
    return rng.integers(LO, HI, (n, 2, 128)).astype(np.int32)


def _assert_mix(ref, what):
    """both sides of every ReLU and every label, on the reference alone"""
    zero_dense = float((ref["dense"] == 0).mean())
    assert 0.10 <= zero_dense <= 0.70, (what, zero_dense)
    assert set(np.unique(ref["labels"]).tolist()) == {0, 1, 2}, what
    assert float((ref["conv"] == 0).mean()) >= 0.30 and float((ref["conv"] > 0).mean()) >= 0.30, what


@functools.lru_cache(maxsize=None)
def _batch(F):
    """(weights, 1,000 frames of uniform 18-bit words, the oracle's result) for the full-range weights of F: computed once, shared
    and left unchanged by every test that uses them"""
    w = _full_range_weights(F, SEED[F])
    x = _words(np.random.default_rng(1000 + SEED[F]), 1000)
    ref = Q.forward_q612(x.astype(np.int64), Q.quantize_weights(w))
    _assert_mix(ref, f"F {F} seed {SEED[F]}")
    x.setflags(write=False)
    return w, x, ref


@functools.lru_cache(maxsize=None)
def _model(F, kind="full"):
    w = _batch(F)[0] if kind == "full" else load_deployed_npz(TRAINED[F])
    m = VTCNN2(Topology.deployed(F, 3))
    m.set_weights(w)
    return m, w


def _run(m, x, n=None, dense=True, labels=True, stream=None):
    """mdc_forward_q612 straight through the binding on a host array or a device tensor (float32 frames or int32 words).  The outputs
    are pre-filled with SENTINEL and carry one guard row / element, checked here.  Returns (dense (n,3), labels (n)) device tensors,
    None for the one not asked for."""
    dev = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.array(x)).cuda()
    assert dev.is_cuda and dev.is_contiguous() and dev.dtype in (torch.float32, torch.int32) and tuple(dev.shape[1:]) == (2, 128)
    n = dev.shape[0] if n is None else n
    d = torch.full((n + 1, 3), SENTINEL, dtype=torch.int32, device="cuda")
    lab = torch.full((n + 1,), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.current_stream() if stream is None else stream
    _cabi.check(_cabi.lib().mdc_forward_q612(m._engine(), dev.data_ptr() if n else None, int(dev.dtype == torch.int32), n,
                                             d.data_ptr() if dense else None, lab.data_ptr() if labels else None, s.cuda_stream))
    s.synchronize()
    torch.cuda.synchronize()
    assert d[n].tolist() == [SENTINEL] * 3 and lab[n].item() == SENTINEL
    if not dense:
        assert (d == SENTINEL).all()
    if not labels:
        assert (lab == SENTINEL).all()
    return (d[:n] if dense else None), (lab[:n] if labels else None)


def _assert_equals_oracle(got, ref, msg=""):
    d, lab = got
    np.testing.assert_array_equal(d.cpu().numpy().astype(np.int64), ref["dense"], err_msg=msg)
    np.testing.assert_array_equal(lab.cpu().numpy(), ref["labels"], err_msg=msg)


def _cut(ref, sel):
    return {"dense": ref["dense"][sel], "labels": ref["labels"][sel]}


# ---------------------------------------------------------------------------------------------------------------- a. every wave, every tail
# F = 10: n >= 129 reaches waves 2 and 3 (one LDS weight region each), n >= 257 a second work-group
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 320, 511, 513, 1000])
@pytest.mark.parametrize("F", [3, 10])
def test_full_range_operands_at_every_block_cut(F, n):
    m, _ = _model(F)
    _, x, ref = _batch(F)
    want = _cut(ref, slice(0, n))
    got = _run(m, x[:n])
    _assert_equals_oracle(got, want, f"F {F} n {n}")
    # the same words with random bits above bit 17: the kernel and the oracle take a word modulo 2^18
    rng = np.random.default_rng(n)
    planted = ((x[:n].astype(np.int64) & 0x3FFFF) | (rng.integers(0, 1 << 14, x[:n].shape) << 18)).astype(np.uint32).view(np.int32)
    np.testing.assert_array_equal(Q.wrap(planted, 18), x[:n])
    assert (planted != x[:n]).mean() > 0.9
    again = _run(m, planted)
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])
    _assert_equals_oracle(again, want, f"F {F} n {n}, bits above 17")


# ---------------------------------------------------------------------------------------------------------------- b. one-hot frames
@pytest.mark.parametrize("F", [3, 10])
def test_one_hot_frames(F):
    m, w = _model(F)
    _batch(F)                                                    # the weights' mix condition
    cols = [0, 1, 2, 63, 64, 125, 126, 127]
    hot = np.zeros((32, 2, 128), np.float32)
    i = 0
    for v in (1.0, -32.0):
        for h in range(2):
            for c in cols:
                hot[i, h, c] = v
                i += 1
    assert i == 32 and ((hot != 0).sum(axis=(1, 2)) == 1).all()
    x = np.concatenate([hot, _words(np.random.default_rng(77), 40).astype(np.float32) / 4096.0])      # one block of 64 and one of 8
    xq = Q.quantize(x)
    assert sorted(np.unique(xq[:32]).tolist()) == [LO, 0, 4096]
    ref = Q.forward_q612(xq, Q.quantize_weights(w))
    assert len({tuple(r) for r in ref["dense"][:32].tolist()}) >= 24      # the hot frames are told apart by the sums
    _assert_equals_oracle(_run(m, x), ref, f"F {F} float frames")
    _assert_equals_oracle(_run(m, xq.astype(np.int32)), ref, f"F {F} integer words")


# ---------------------------------------------------------------------------------------------------------------- c. float quantisation
def _below(v):
    return float(np.nextafter(np.float32(v), np.float32(0)))


EDGES = [0.0, -0.0, 2.0 ** -12, -2.0 ** -12, _below(2.0 ** -12), -_below(2.0 ** -12), 1e-40, -1e-40,
         32 - 2.0 ** -12, 32.0, -32.0, -32 - 2.0 ** -12, _below(2.0 ** 19), -_below(2.0 ** 19)]


@functools.lru_cache(maxsize=None)
def _float_frames():
    """200 frames: magnitudes log-uniform over [2^-14, 2^19), random sign, and in every frame the EDGES at random places (frame 0:
    from column 0 on, frame 1: up to column 127 of row 1)"""
    assert _below(2.0 ** 19) == 524287.96875 and np.float32(1e-40) != 0 and abs(np.float32(1e-40)) < np.finfo(np.float32).tiny
    rng = np.random.default_rng(19)
    n = 200
    x = (2.0 ** rng.uniform(-14, 19, (n, 256))).astype(np.float32)
    x = np.minimum(x, np.float32(_below(2.0 ** 19))) * rng.choice(np.array([-1, 1], np.float32), (n, 256))
    edges = np.array(EDGES, np.float32)
    for i in range(n):
        at = np.arange(len(edges)) if i == 0 else 256 - len(edges) + np.arange(len(edges)) if i == 1 else rng.choice(256, len(edges), replace=False)
        x[i, at] = rng.permutation(edges) if i > 1 else edges
    x = x.reshape(n, 2, 128)
    assert np.abs(x).max() < 2.0 ** 19 and np.isfinite(x).all()
    q = Q.quantize(x)
    assert q.min() == LO and q.max() == HI - 1 and (q == 0).sum() >= 4 * n       # the whole range comes out; +-0, +-(2^-12 - ulp), denormal
    x.setflags(write=False)
    return x, q


def test_quantize_edges_on_the_oracle_side():
    """what the EDGES must become (float2fix: truncate toward zero, wrap to 18 bits): the reference of the test below"""
    assert Q.quantize(np.array(EDGES, np.float32)).tolist() == [0, 0, 1, -1, 0, 0, 0, 0, HI - 1, LO, LO, HI - 1, -128, 128]      # 2^19 - 2^-5 -> 2^31 - 128


@pytest.mark.parametrize("kind", ["trained", "full"])
@pytest.mark.parametrize("F", [3, 10])
def test_float_quantisation_up_to_2_19(F, kind):
    m, w = _model(F, kind)
    if kind == "full":
        _batch(F)
    x, q = _float_frames()
    ref = Q.forward_from_float(x, w)
    got = _run(m, x)
    _assert_equals_oracle(got, ref, f"F {F} {kind} weights, float frames")
    words = _run(m, q.astype(np.int32))
    assert torch.equal(words[0], got[0]) and torch.equal(words[1], got[1])


# ---------------------------------------------------------------------------------------------------------------- d. outside the domain
@pytest.mark.parametrize("F", [3, 10])
def test_frames_outside_the_domain_stay_to_themselves(F):
    """include/mdc.h: a frame with a NaN, an infinity or |v| >= 2^19 has unspecified sums and a label in [0, 3), and never affects
    another frame -- not through the one-frame-ahead prefetch, the lane that parks its totals or the block it shares"""
    m, w = _model(F)
    _, xw, ref = _batch(F)
    n = 300
    x = xw[:n].astype(np.float32) / 4096.0
    bad_frames = [0, 1, 63, 64, 65, 191, 299]
    bad_values = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 2.0 ** 19, -2.0 ** 19], np.float32)
    rng = np.random.default_rng(23)
    xb = x.copy()
    for k, i in enumerate(bad_frames):
        v = np.roll(bad_values, k)[:3 + k % 4]
        if k == 0:
            xb[i] = np.resize(bad_values, 256).reshape(2, 128)            # a whole frame of them
        else:
            xb[i].reshape(-1)[rng.choice(256, v.size, replace=False)] = v
        xb[i, k % 2, [0, 127][k % 2]] = bad_values[k]                   # and one at an end of a row
    good = np.setdiff1d(np.arange(n), bad_frames)
    assert (xb[good] == x[good]).all() and all((~np.isfinite(xb[i]) | (np.abs(xb[i]) >= 2.0 ** 19)).any() for i in bad_frames)
    clean = _run(m, x)
    _assert_equals_oracle(clean, _cut(ref, slice(0, n)), f"F {F}")
    dirty = _run(m, xb)
    g = torch.from_numpy(good).cuda()
    assert torch.equal(dirty[0][g], clean[0][g]) and torch.equal(dirty[1][g], clean[1][g])
    lab = dirty[1].cpu().numpy()
    assert ((lab >= 0) & (lab < 3)).all()


# ---------------------------------------------------------------------------------------------------------------- e. past the grid cap
@pytest.mark.parametrize("F", [3, 10])
def test_the_walk_past_the_grid_cap(F):
    """the smallest n that takes a second pass: three whole blocks and one of 37 frames beyond what the capped grid covers at once"""
    m, w = _model(F)
    block = _cabi.Q612_BLOCK_FRAMES
    cover = _cabi.Q612_GRID_CAP * 4 * block
    n = cover + 3 * block + 37
    assert n > cover and block == 64
    gen = torch.Generator(device="cuda")
    gen.manual_seed(612 + F)
    x = torch.randint(LO, HI, (n, 2, 128), dtype=torch.int32, device="cuda", generator=gen)
    dense, labels = _run(m, x)
    rng = np.random.default_rng(F)
    picks = np.unique(np.concatenate([np.arange(70), np.arange(cover - 70, cover + 70), np.arange(n - 70, n), rng.integers(0, n, 1000)]))
    assert picks.size <= 1400 and (picks < cover).sum() >= 500 and (picks >= cover).sum() >= 140
    assert {cover - 1, cover, cover + 3 * block - 1, cover + 3 * block, n - 1} <= set(picks.tolist())      # the picks straddle the seam
    p = torch.from_numpy(picks).cuda()
    ref = Q.forward_q612(x[p].cpu().numpy().astype(np.int64), Q.quantize_weights(w))
    _assert_mix(ref, f"F {F} picks")
    _assert_equals_oracle((dense[p], labels[p]), ref, f"F {F} n {n}")
    # every other frame: against a two-piece run whose second piece starts off the 64-frame grid, so that each of its blocks is cut
    # differently and (being far under the cap) is handled in one pass
    a = cover // 4 * 3 + 23
    assert a % block != 0 and 0 < n - a <= cover
    d1, l1 = _run(m, x[:a])
    d2, l2 = _run(m, x[a:])
    assert torch.equal(torch.cat([d1, d2]), dense) and torch.equal(torch.cat([l1, l2]), labels)


# ---------------------------------------------------------------------------------------------------------------- f. ties
@pytest.mark.parametrize("F", [3, 10])
def test_first_maximum_wins_a_tie_of_equal_positive_sums(F):
    (ck, cb), (dk, db) = _full_range_weights(F, 40 + F)
    dk, db = dk.copy(), db.copy()
    dk[:, 2] = dk[:, 1]
    db[2] = db[1]
    db[0] = LO / 4096.0
    w = [(ck, cb), (dk, db)]
    n = 300
    x = _words(np.random.default_rng(41 + F), n)
    x[7] = 0
    ref = Q.forward_q612(x.astype(np.int64), Q.quantize_weights(w))
    s = ref["dense"]
    assert (s[:, 1] == s[:, 2]).all()
    tie = (s[:, 1] > 0) & (s[:, 1] > s[:, 0])
    allzero = (s == 0).all(axis=1)
    assert tie.sum() >= 20 and allzero.sum() >= 1 and ((s[:, 0] > s[:, 1]).sum() >= 1)
    assert (ref["labels"][tie] == 1).all() and (ref["labels"][allzero] == 0).all()
    m = VTCNN2(Topology.deployed(F, 3))
    m.set_weights(w)
    got = _run(m, x)
    _assert_equals_oracle(got, ref, f"F {F}")
    lab = got[1].cpu().numpy()
    assert (lab[tie] == 1).all() and (lab[allzero] == 0).all() and not (lab == 2).any()


# ---------------------------------------------------------------------------------------------------------------- g. ABI corners
def test_null_outputs_and_a_side_stream():
    m, _ = _model(3)
    _, x, ref = _batch(3)
    n = 321
    want = _cut(ref, slice(0, n))
    both = _run(m, x[:n])
    _assert_equals_oracle(both, want)
    _, only_labels = _run(m, x[:n], dense=False)
    only_dense, _ = _run(m, x[:n], labels=False)
    assert torch.equal(only_labels, both[1]) and torch.equal(only_dense, both[0])
    side = torch.cuda.Stream()
    assert side.cuda_stream != torch.cuda.current_stream().cuda_stream
    on_side = _run(m, x[:n], stream=side)
    assert torch.equal(on_side[0], both[0]) and torch.equal(on_side[1], both[1])


def test_five_filters_are_refused():
    """the deployed kernels, this one included, are instantiated for F = 3 and F = 10 (every bundled checkpoint has one of the two).
    A deployed topology with another F never becomes a model: mdc_create refuses it with MDC_ENOTSUP and a message that names both,
    so predict_q612 raises before any handle exists and nothing can be launched on its behalf"""
    import ctypes
    m = VTCNN2(Topology.deployed(5, 3))
    m.set_weights(_full_range_weights(5, 5))
    assert m.topology.filters == 5 and m.topology.classes == 3
    lib = _cabi.lib()
    topo = _cabi.MdcTopology(_cabi.KIND_DEPLOYED, 5, 0, 3, (ctypes.c_int32 * 4)(0, 0, 0, 0))
    h = ctypes.c_void_p()
    rc = lib.mdc_create(ctypes.byref(topo), torch.cuda.current_device(), ctypes.byref(h))
    assert rc == ENOTSUP and not h.value                                  # no model: nothing to launch with
    msg = lib.mdc_last_error().decode()
    assert "3 or 10" in msg and "got 5" in msg, msg
    n = 70
    with pytest.raises(_cabi.MdcError) as e:
        m.predict_q612(np.zeros((n, 2, 128), np.float32))
    assert e.value.code == ENOTSUP and "3 or 10" in str(e.value)
    with pytest.raises(_cabi.MdcError) as e:
        m.predict_q612(torch.zeros((n, 2, 128), dtype=torch.int32, device="cuda"), as_float=False)
    assert e.value.code == ENOTSUP and m._handle is None
    # a NULL model is refused by mdc_forward_q612 itself, with the outputs untouched
    d = torch.full((n, 3), SENTINEL, dtype=torch.int32, device="cuda")
    lab = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
    x = torch.zeros((n, 2, 128), dtype=torch.int32, device="cuda")
    assert lib.mdc_forward_q612(None, x.data_ptr(), 1, n, d.data_ptr(), lab.data_ptr(), torch.cuda.current_stream().cuda_stream) < 0
    torch.cuda.synchronize()
    assert (d == SENTINEL).all() and (lab == SENTINEL).all()
