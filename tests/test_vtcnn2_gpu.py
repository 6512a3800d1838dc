"""Parity of the canonical VT-CNN2 HIP path (conv1+conv2 MFMA kernel, dense1 GEMM, softmax head)
against the CPU oracle, through the C ABI.  No reference outputs exist for this topology (no
weights are bundled): parity is against this repo's f64 oracle ("parity unpinned").  The weights here are the untrained
synthetic draws; the same bars, a per-frame bar and the label floors are held on a TRAINED net (matched conv2 filters,
decisive and thin margins) in tests/test_trained_vtcnn2_gpu.py (profiles/r06_measured_bars.json).

Tolerances (relative to the largest |logit| of the batch, since the net is positively
homogeneous in its input scale):
  f32 path : 2e-5   (exact-f32 MFMA fma chains, K up to 10560)
  bf16 path: 8e-3   (bf16 operands, f32 accumulation; the largest error over this file's scenarios is 3.8e-3 on the logits,
                     4.0e-3 on the features, 8e-4 on the probabilities: tools/measure_bars.py -> profiles/r03_measured_bars.json)
  fp8 path : 5e-2   (conv2 on e4m3 operands, measured 4.0e-2 / 3.7e-2 / 1.2e-2; activations scaled for a stated input range;
                     round 4: E4M3 features between conv2 and dense1 as well -- the 'flat' / 'conv' taps carry that rounding, v/16)
i.e. about twice (fp8: 1.25 x) what is measured -- round 2's 2e-2 / 8e-2 would have passed a kernel three times as wrong.
Probabilities: half the logit bar (softmax contracts).  Labels: bit-exact wherever the oracle's top-2 logit margin
exceeds 4x the tolerance; every frame counts in tests/test_label_agreement_gpu.py.
Faults too small for these bars are caught in tests/test_exact_fixtures_gpu.py (integer fixtures, bit-for-bit against the oracle)."""
import ctypes

import numpy as np
import pytest
import torch

from modulationdetectioncnn_amd import VTCNN2, Topology, _cabi, synthetic_frames, synthetic_weights
from oracle import oracle_np as O

pytestmark = pytest.mark.gpu

TOL = {"f32": 2e-5, "bf16": 8e-3, "fp8": 5e-2}
_cache = {}


def _setup(classes, seed=2016, bias_scale=0.0):
    key = (classes, seed, bias_scale)
    if key not in _cache:
        topo = Topology.vtcnn2(classes)
        _cache[key] = (topo, synthetic_weights(topo, seed=seed, bias_scale=bias_scale))
    return _cache[key]


def _model(classes, dtype, fp8_input_absmax=None, **kw):
    topo, w = _setup(classes, **kw)
    m = VTCNN2(topo, dtype=dtype, fp8_input_absmax=fp8_input_absmax if dtype == "fp8" else None)
    m.set_weights(w)
    return m, w


def _check(m, w, x, dtype, batch_size=None):
    ref = O.forward("vtcnn2", x, w, dtype=np.float64)
    scale = float(np.abs(ref["logits"]).max())
    tol = TOL[dtype]
    lg = m.predict(x, tap="dense", batch_size=batch_size)
    assert np.abs(lg - ref["logits"]).max() <= tol * scale, (np.abs(lg - ref["logits"]).max() / scale)
    p = m.predict(x, batch_size=batch_size)
    assert np.abs(p - ref["probs"]).max() <= max(2e-6, (2 if dtype == "f32" else 0.5) * tol * scale)
    np.testing.assert_allclose(p.sum(axis=1), 1.0, atol=1e-5)
    lab = m.predict_classes(x, batch_size=batch_size)
    srt = np.sort(ref["logits"], axis=1)
    decided = (srt[:, -1] - srt[:, -2]) > 4 * tol * scale
    assert (lab[decided] == ref["labels"][decided]).all()
    # argmax must be the first max of OUR probabilities
    assert (lab == np.argmax(p, axis=1)).all()
    return ref, decided.mean()


@pytest.mark.parametrize("dtype", ["f32", "bf16", "fp8"])
@pytest.mark.parametrize("classes", [3, 11])
@pytest.mark.parametrize("n", [1, 16, 17, 64, 100, 257])
def test_parity(dtype, classes, n):
    m, w = _model(classes, dtype)
    x = synthetic_frames(n, seed=2016)
    _check(m, w, x, dtype)


@pytest.mark.parametrize("dtype", ["f32", "bf16", "fp8"])
def test_parity_with_biases_and_large_inputs(dtype):
    x = synthetic_frames(96, seed=7, sigma=0.5)
    m, w = _model(11, dtype, seed=5, bias_scale=0.05, fp8_input_absmax=float(np.abs(x).max()))
    _check(m, w, x, dtype)


@pytest.mark.parametrize("dtype", ["f32", "bf16", "fp8"])
def test_taps(dtype):
    x = synthetic_frames(40, seed=3, sigma=0.1)
    m, w = _model(11, dtype, seed=5, bias_scale=0.05, fp8_input_absmax=float(np.abs(x).max()))
    ref = O.forward("vtcnn2", x, w, dtype=np.float64, taps=True)
    tol = TOL[dtype]
    flat = m.predict(x, tap="flat")
    assert flat.shape == (40, 10560)
    # fp8 mode (round 4): the features themselves are E4M3 values (x a power of two), rounded to nearest on a grid whose
    # spacing is 1/8 of the binade's base: half a spacing = at most 1/16 of the value at the bottom of a binade, 1/32 at the
    # top -- on top of the conv's own error.  Bar: tol + 1/32 of the largest feature (round 4 allowed tol + 1/16 after a red
    # run; measured 6.06 % with E4M3 features, 3.7 % with bf16 features: profiles/r05_measured_bars.json)
    flat_tol = tol + (1.0 / 32 if dtype == "fp8" else 0.0)
    assert np.abs(flat - ref["flat"]).max() <= flat_tol * np.abs(ref["flat"]).max()
    conv = m.predict(x, tap="conv")
    assert conv.shape == (40, 80, 132)
    np.testing.assert_array_equal(conv.reshape(40, -1), flat)
    hid = m.predict(x, tap="hidden")
    assert hid.shape == (40, 256)
    assert np.abs(hid - ref["dense1"]).max() <= tol * np.abs(ref["dense1"]).max()


@pytest.mark.parametrize("dtype", ["f32", "bf16", "fp8"])
def test_batch_size_invariance(dtype):
    m, w = _model(11, dtype)
    x = synthetic_frames(300, seed=11, device="cuda")
    a = m.predict(x)
    for bs in (16, 100, 299):
        assert torch.equal(a, m.predict(x, batch_size=bs))
    la = m.predict_classes(x)
    assert torch.equal(la, m.predict_classes(x, batch_size=64))


def test_zero_input_and_relu_exact_zero():
    # zero frames, zero biases: every activation is exactly 0 -> logits 0 -> uniform softmax, label 0
    for dtype in ("f32", "bf16", "fp8"):
        m, _ = _model(11, dtype)
        x = np.zeros((20, 2, 128), np.float32)
        p = m.predict(x)
        np.testing.assert_array_equal(p, np.full((20, 11), np.float32(1.0) / np.float32(11.0)))
        assert (m.predict_classes(x) == 0).all()


def test_f32_larger_batch_statistics():
    m, w = _model(3, "f32")
    x = synthetic_frames(1500, seed=99)
    _, frac = _check(m, w, x, "f32")
    assert frac > 0.999


def test_fp8_feature_formats():
    """MDC_FP8 keeps its conv2 features as E4M3 bytes (the default since ABI 4: 11,584 workspace bytes per frame) or, with
    MDC_OPT_FP8_BF16_FEATURES, as bf16 (22,144: rounds 1-3).  Every value of the E4M3 'flat' tap is an E4M3 number times
    ONE power of two; both formats meet the mode's logit bar against the f64 oracle, and the bf16 one is closer on the
    features (8 significant bits instead of 4); the option is refused outside the fp8 mode."""
    x = synthetic_frames(512, seed=21)
    topo = Topology.vtcnn2(11)
    w = synthetic_weights(topo, seed=2016)
    ref = O.forward("vtcnn2", x, w, dtype=np.float64)
    scale = np.abs(ref["logits"]).max()
    errs = {}
    for bf in (False, True):
        m = VTCNN2(topo, dtype="fp8", fp8_bf16_features=bf)
        m.set_weights(w)
        lg = m.predict(x, tap="dense")
        errs[bf] = float(np.abs(lg - ref["logits"]).max() / scale)
        assert errs[bf] <= TOL["fp8"], (bf, errs[bf])
        per_frame = _cabi.lib().mdc_workspace_bytes(m._engine(), 1 << 16) / (1 << 16)
        assert per_frame == (22144 if bf else 11584)
        flat = m.predict(x[:64], tap="flat").astype(np.float64)
        nz = flat[flat > 0]
        # mantissa of every feature in the E4M3 grid: v = m * 2^e with m in {8..15}/8 (normals) -- i.e. v / 2^floor(log2 v) * 8 is an integer
        frac = nz / 2.0 ** np.floor(np.log2(nz)) * 8
        on_grid = np.abs(frac - np.round(frac)) < 1e-9
        assert on_grid.all() == (not bf), (bf, on_grid.mean())      # (e4m3 subnormals are on that grid too; bf16 features are not)
        ferr = float(np.abs(flat - ref["flat"][:64]).max() / np.abs(ref["flat"][:64]).max())
        errs[("flat", bf)] = ferr
        # the batch kernels (n > 2,048: asm conv loop, phased dense1 with the fused head) and the small-batch forms
        # (position-range conv, per-wave / four-wave dense1) of THIS feature format give the same bits
        xb = synthetic_frames(5000, seed=22, device="cuda")
        big = m.predict(xb)
        for k in (1, 200, 1500):
            assert torch.equal(big[:k], m.predict(xb[:k].contiguous())), (bf, k)
    assert errs[("flat", True)] < errs[("flat", False)] <= TOL["fp8"] + 1 / 16
    with pytest.raises(ValueError):
        VTCNN2(topo, dtype="bf16", fp8_bf16_features=True)
    t = _cabi.MdcTopology(2, 256, 256, 11, (ctypes.c_int32 * 4)(_cabi.MDC_OPT_FP8_BF16_FEATURES, 0, 0, 0))
    h = ctypes.c_void_p()
    L = _cabi.lib()
    assert L.mdc_create(ctypes.byref(t), 0, ctypes.byref(h)) == 0
    try:
        for i, (k, b) in enumerate(w):
            assert L.mdc_set_weights(h, i, k.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), k.size, b.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), b.size) == 0
        L.mdc_last_error.restype = ctypes.c_char_p
        assert L.mdc_finalize(h, 1) == -22 and b"MDC_FP8" in L.mdc_last_error()      # the option at MDC_BF16
    finally:
        L.mdc_destroy(h)


def test_fp8_rejects_other_topologies_and_bad_scale():
    m = VTCNN2.synthetic("cnnpy", classes=5, dtype="fp8")          # fp8: vtcnn2 and deployed, not the cnn.py literal model
    with pytest.raises(Exception):
        m.predict(np.zeros((1, 2, 128), np.float32))
    topo, wv = _setup(3)
    bad = VTCNN2(topo, dtype="fp8", fp8_input_absmax=-1.0)
    bad.set_weights(wv)
    with pytest.raises(Exception):
        bad.predict(np.zeros((1, 2, 128), np.float32))


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_ragged_batch_sizes_against_the_f32_kernels(dtype):
    """Every batch size 1..48 plus the group / tile / grid boundaries (16-frame groups, 256-row GEMM tiles, 256
    persistent work-groups): the MFMA paths against the exact-f32 path, frame by frame."""
    mf, _ = _model(11, "f32")
    m, _ = _model(11, dtype)
    tol = TOL[dtype]
    x_all = synthetic_frames(8200, seed=21, device="cuda")
    ref_all = mf.predict(x_all, tap="dense")
    scale = float(ref_all.abs().max())
    for n in list(range(1, 49)) + [255, 256, 257, 511, 513, 4095, 4096, 4097, 4113, 8200]:
        got = m.predict(x_all[:n].contiguous(), tap="dense")
        assert got.shape == (n, 11)
        assert float((got - ref_all[:n]).abs().max()) <= tol * scale, n


def test_fp8_saturates_instead_of_nan_beyond_the_stated_range():
    m, _ = _model(11, "fp8")                       # scaled for |x| <= 0.02
    x = synthetic_frames(32, seed=3, sigma=0.5)      # 25x larger
    p = m.predict(x)
    assert np.isfinite(p).all()
    np.testing.assert_allclose(p.sum(axis=1), 1.0, atol=1e-5)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_two_streams_share_one_model(dtype):
    """mdc_forward is re-entrant on a finalized model (include/mdc.h): forwards of one model enqueued on two HIP
    streams at once, each with its own workspace, give exactly what they give one after the other."""
    m = VTCNN2.synthetic(Topology.vtcnn2(11), seed=2016, device=0, dtype=dtype)
    n = 8192 if dtype == "bf16" else 2048
    xa = synthetic_frames(n, seed=21, device="cuda:0")
    xb = synthetic_frames(n, seed=22, device="cuda:0")
    pa, la, _ = m.forward_device(xa, batch_size=1024)
    pb, lb, _ = m.forward_device(xb, batch_size=1024)
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(3):
        with torch.cuda.stream(sa):
            qa, ka, _ = m.forward_device(xa, batch_size=1024)
        with torch.cuda.stream(sb):
            qb, kb, _ = m.forward_device(xb, batch_size=1024)
        torch.cuda.synchronize()
        assert torch.equal(qa, pa) and torch.equal(ka, la) and torch.equal(qb, pb) and torch.equal(kb, lb)
    assert len(m._ws) == 3          # default stream + the two above: one scratch buffer each


@pytest.mark.parametrize("dtype", ["f32", "bf16", "fp8"])
def test_small_batch_forms_are_bit_identical_to_the_batch_kernels(dtype):
    """A single window (or a few) takes other launch forms -- one conv position per work-group in f32, a range of 12
    positions per work-group in bf16 / fp8 (up to 1,024 frames), a per-wave dense1 tile in every dtype (up to 2,048)
    -- that run the same instruction sequence per output element: a frame's result must
    not depend on how many frames it arrives with.  (The reference classifies one window per start pulse,
    cnn_test_latest1.sv:144-209.)"""
    m, _ = _model(11, dtype)
    # f32 (round 5): dense1 takes 64-row tiles up to 16,384 frames and 128-row tiles beyond -- the big batch is the 128-row form
    nbig = 20000 if dtype == "f32" else 9000
    x = synthetic_frames(nbig, seed=31, device="cuda")
    big_p, big_l, _ = m.forward_device(x, batch_size=nbig)            # batch kernels (n > 8,192; f32: > 16,384)
    big_h = m.predict(x, tap="hidden", batch_size=nbig)
    sizes = (1, 2, 15, 16, 17, 33, 64, 65, 128, 129, 300, 1009, 1024, 1025, 2048, 2049, 4097, 8192, 8193) + ((16384, 16385) if dtype == "f32" else ())
    for n in sizes:      # every launch form and its boundaries
        xs = x[:n].contiguous()
        p, l, _ = m.forward_device(xs)
        assert torch.equal(p, big_p[:n]) and torch.equal(l, big_l[:n]), (dtype, n)
        assert torch.equal(m.predict(xs, tap="hidden"), big_h[:n]), (dtype, n)
    # a window taken from the middle of the batch, alone
    one = x[4321:4322].contiguous()
    assert torch.equal(m.forward_device(one)[0], big_p[4321:4322])


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("classes", [3, 11, 16])
def test_head_fused_into_dense1_gives_the_bits_of_the_separate_launch(dtype, classes):
    """Round 3: above 2,048 frames the 16-bit modes run dense2 + softmax + argmax inside the dense1 GEMM's epilogue (no
    hidden layer in HBM).  A forward that taps the logits takes the unfused path (dense1 writes the hidden layer, the head
    is its own launch): probabilities and labels must be the same BITS -- ragged sizes around the 256-row tile included --
    and so must the small-batch forms' (the first 2,048 frames of the same batch)."""
    m, _ = _model(classes, dtype, seed=5, bias_scale=0.05)
    x = synthetic_frames(2 * 4096 + 17, seed=31, device="cuda")
    for n in (2049, 2304, 4096, 4097, 2 * 4096 + 17):
        xn = x[:n].contiguous()
        p_f, l_f, _ = m.forward_device(xn)
        p_s, l_s, logits = m.forward_device(xn, tap="dense")
        assert torch.equal(p_f, p_s) and torch.equal(l_f, l_s), (n, classes)
        assert logits.shape == (n, classes)
        hid = m.predict(xn, tap="hidden")
        assert hid.shape == (n, 256) and bool(torch.isfinite(hid).all())
    small = m.forward_device(x[:2048].contiguous())
    big = m.forward_device(x[:4096].contiguous())
    assert torch.equal(small[0], big[0][:2048]) and torch.equal(small[1], big[1][:2048])
    # only probabilities, only labels
    xn = x[:3000].contiguous()
    p_ref, l_ref, _ = m.forward_device(xn)
    L, h = m._lib(), m._engine()
    ws, nb = m._workspace(3000)
    stream = torch.cuda.current_stream().cuda_stream
    p2 = torch.empty_like(p_ref)
    l2 = torch.empty_like(l_ref)
    m._check(L.mdc_forward(h, xn.data_ptr(), 3000, p2.data_ptr(), None, None, 0, ws.data_ptr(), nb, stream))
    m._check(L.mdc_forward(h, xn.data_ptr(), 3000, None, l2.data_ptr(), None, 0, ws.data_ptr(), nb, stream))
    assert torch.equal(p2, p_ref) and torch.equal(l2, l_ref)


def test_default_workspace_is_bounded_and_old_streams_do_not_pin_hbm():
    """VERDICT r2 item 6 / ADVICE: predict() on a large batch must not ask for 21 KB x 2^20 of scratch per stream by default
    -- 65,536-frame calls, < 4 GB at f32, 1.45 GB in the 16-bit modes -- with results identical to the one-launch form a
    caller opts into with batch_size; at most MAX_WORKSPACES scratch buffers stay alive however many streams came by."""
    m, _ = _model(11, "bf16")
    assert m.default_chunk == 1 << 16
    x = synthetic_frames(3 * 65536 + 5, seed=8, device="cuda")
    p = m.predict(x)
    assert sum(t.numel() for t in m._ws.values()) < 2 * 1024 ** 3
    assert torch.equal(p, m.predict(x, batch_size=x.shape[0]))
    mf, _ = _model(3, "f32")
    mf.predict(x[:70000].contiguous())
    assert sum(t.numel() for t in mf._ws.values()) < 4 * 1024 ** 3
    m2, _ = _model(11, "bf16")
    outs = []
    for _ in range(7):
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            outs.append(m2.predict(x[:4096]))
        st.synchronize()
    assert len(m2._ws) <= m2.MAX_WORKSPACES == 4
    assert all(torch.equal(o, outs[0]) for o in outs)
