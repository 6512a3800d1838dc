"""Non-finite input frames (cnn.py:153, 198): mdc_forward_checked / mdc_predict_host_checked flag exactly the frames that hold
a NaN or +-Inf sample, leave every result bit-identical to mdc_forward under REPORT, and give the flagged frames Keras'
all-NaN row and np.argmax's label 0 under PROPAGATE -- for every kind and dtype, at group and tail boundaries."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from modulationdetectioncnn_amd import NonFiniteInputError, Topology, VTCNN2, _cabi, synthetic_frames, synthetic_weights  # noqa: E402

CASES = [("deployed3", "f32"), ("deployed3", "bf16"), ("deployed3", "f16"), ("deployed3", "fp8"),
         ("deployed10", "f32"), ("deployed10", "bf16"), ("deployed10", "f16"), ("deployed10", "fp8"),
         ("vtcnn2", "f32"), ("vtcnn2", "bf16"), ("vtcnn2", "fp8"), ("vtcnn2", "fp8_bf16"), ("cnnpy", "f32")]
SIZES = [1, 15, 16, 17, 4100, 65539]
FMAX = np.finfo(np.float32).max
# (row, position, value): single bad samples at the staging edges, then whole-NaN frames (row None)
BAD = [(0, 0, np.nan), (1, 127, np.inf), (0, 127, -np.inf), (1, 0, np.nan), (0, 0, np.inf), (1, 127, -np.inf),
       (None, None, np.nan), (0, 127, np.nan), (1, 0, -np.inf)]
# finite extremes that must NOT be flagged
FINITE = [FMAX, -FMAX, np.float32(1e-40), np.float32(-0.0), np.float32(1e30), -np.float32(1e30)]

_models = {}


def _model(topo, dtype):
    key = (topo, dtype)
    if key not in _models:
        t = Topology.vtcnn2(11) if topo == "vtcnn2" else topo
        kw = {"dtype": "fp8", "fp8_bf16_features": True} if dtype == "fp8_bf16" else {"dtype": dtype}
        _models.clear()                        # one model (and its workspaces) alive at a time
        _models[key] = VTCNN2.synthetic(t, seed=2016, device=0, **kw)
    return _models[key]


def _frames(n, seed=5):
    """synthetic frames with bad samples at the group / tail edges and finite extremes next to them; returns (x, bad frames)"""
    x = synthetic_frames(n, seed=seed)
    where = sorted({i for i in (0, 1, 14, 15, 16, 17, 63, 64, 255, 256, 4095, 4096, 16383, 16384, 16385, 65535, 65536, n // 2, n - 2, n - 1) if 0 <= i < n})
    bad = where[::2]
    for k, i in enumerate(bad):
        r, p, v = BAD[k % len(BAD)]
        if r is None:
            x[i] = v
        else:
            x[i, r, p] = v
    for k, i in enumerate(where[1::2]):
        x[i, k % 2, (0, 127, 64)[k % 3]] = FINITE[k % len(FINITE)]
    return x, bad


def _checked(m, xd, policy, flags=None, count=None, probs=None, labels=None):
    n = xd.shape[0]
    dev = xd.device
    probs = torch.full((n, m.topology.classes), -7.0, device=dev) if probs is None else probs
    labels = torch.full((n,), -7, dtype=torch.int32, device=dev) if labels is None else labels
    flags = torch.full((n,), 9, dtype=torch.uint8, device=dev) if flags is None else flags
    count = torch.zeros((1,), dtype=torch.int64, device=dev) if count is None else count
    ws, ws_bytes = m._workspace(max(n, 1))
    _cabi.check(_cabi.lib().mdc_forward_checked(m._engine(), xd.data_ptr(), n, probs.data_ptr(), labels.data_ptr(),
                                                ws.data_ptr() if ws is not None else None, ws_bytes, flags.data_ptr(), count.data_ptr(),
                                                policy, torch.cuda.current_stream().cuda_stream))
    return probs, labels, flags, count


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


@pytest.mark.parametrize("topo,dtype", CASES)
@pytest.mark.parametrize("n", SIZES)
def test_flags_report_and_propagate(topo, dtype, n):
    m = _model(topo, dtype)
    x, bad = _frames(n)
    want = ~np.isfinite(x).all(axis=(1, 2))
    assert sorted(np.flatnonzero(want).tolist()) == bad
    xd = torch.from_numpy(x).cuda()
    p0, l0, _ = m.forward_device(xd)
    # REPORT: exact flags, a count that accumulates over two calls, results bit for bit mdc_forward's
    p1, l1, f1, c = _checked(m, xd, _cabi.NONFINITE_REPORT)
    _checked(m, xd, _cabi.NONFINITE_REPORT, count=c)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(f1.cpu().numpy(), want.astype(np.uint8))
    assert int(c.item()) == 2 * int(want.sum())
    np.testing.assert_array_equal(_bits(p1), _bits(p0))
    assert torch.equal(l1, l0)
    # PROPAGATE: clean rows unchanged, flagged rows all NaN with label 0
    p2, l2, f2, c2 = _checked(m, xd, _cabi.NONFINITE_PROPAGATE)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(f2.cpu().numpy(), want.astype(np.uint8))
    assert int(c2.item()) == int(want.sum())
    clean = torch.from_numpy(~want).cuda()
    np.testing.assert_array_equal(_bits(p2[clean]), _bits(p0[clean]))
    assert torch.equal(l2[clean], l0[clean])
    pb = p2[~clean].cpu().numpy()
    assert np.isnan(pb).all() and (l2[~clean].cpu().numpy() == 0).all()


@pytest.mark.filterwarnings("ignore:invalid value encountered")
@pytest.mark.parametrize("topo", ["deployed3", "deployed10", "vtcnn2", "cnnpy"])
def test_propagate_agrees_with_the_f64_oracle_on_nan_frames(topo):
    """A NaN sample gives the f64 oracle (Keras' operation order) an all-NaN row whose argmax is 0: PROPAGATE's row.  For
    +-Inf samples the oracle's rows are reported, not asserted (include/mdc.h: a rectified -Inf can stay finite)."""
    from oracle import oracle_np as O
    m = _model(topo, "f32")
    x, bad = _frames(300)
    rows = np.array(bad)
    ref = O.forward(m.topology.kind, x[rows], synthetic_weights(m.topology, 2016), dtype=np.float64)["probs"]
    nan_frames = np.isnan(x[rows]).any(axis=(1, 2))
    assert nan_frames.any() and (~nan_frames).any()
    assert np.isnan(ref[nan_frames]).all() and (np.argmax(ref[nan_frames], axis=1) == 0).all()
    print(f"{topo}: {int(np.isnan(ref[~nan_frames]).all(axis=1).sum())} of {int((~nan_frames).sum())} +-Inf frames give the oracle a NaN row")
    p, l, _f, _c = _checked(m, torch.from_numpy(x).cuda(), _cabi.NONFINITE_PROPAGATE)
    assert np.isnan(p.cpu().numpy()[rows]).all() and (l.cpu().numpy()[rows] == 0).all()


@pytest.mark.parametrize("topo,dtype", [("deployed3", "f32"), ("deployed10", "bf16"), ("vtcnn2", "bf16"), ("vtcnn2", "fp8"), ("cnnpy", "f32")])
def test_python_surface_equals_the_device_entry(topo, dtype):
    m = _model(topo, dtype)
    n = 70001
    x, bad = _frames(n, seed=9)
    xd = torch.from_numpy(x).cuda()
    for nonfinite, policy in (("propagate", _cabi.NONFINITE_PROPAGATE),):
        p, l, f, _ = _checked(m, xd, policy)
        pn, ln = p.cpu().numpy(), l.cpu().numpy()
        # numpy (host driver) and torch in; chunk sizes that split right next to a bad frame
        for bs in (None, 16384, 16385, 65536):
            np.testing.assert_array_equal(m.predict(x, batch_size=bs, nonfinite=nonfinite).view(np.int32), pn.view(np.int32))
        for bs in (16384, 16385, 65535):        # slots that end at / next to the bad frames 16383..16385, 65535, 65536
            hp, hl = m.predict_host(x, batch_size=bs, nonfinite=nonfinite)
            np.testing.assert_array_equal(hp.view(np.int32), pn.view(np.int32))
            np.testing.assert_array_equal(hl, ln)
        np.testing.assert_array_equal(m.predict(xd, nonfinite=nonfinite).view(torch.int32).cpu().numpy(), pn.view(np.int32))
        np.testing.assert_array_equal(m.predict_classes(x, nonfinite=nonfinite), ln)
        np.testing.assert_array_equal(m.predict_classes(xd, nonfinite=nonfinite).cpu().numpy(), ln)
        fo = torch.zeros((n,), dtype=torch.uint8, device="cuda")
        _p, _l, tap_out = m.forward_device(xd, nonfinite=nonfinite, nonfinite_out=fo)
        assert tap_out is None and torch.equal(fo, f)
    # the library's chunked host driver, chunk sizes at and next to the bad frames, against the device entry
    L = _cabi.lib()
    p, l, f, _ = _checked(m, xd, _cabi.NONFINITE_PROPAGATE)
    for chunk in (1, 16, 17, 4095, 65536, 0):
        hp = np.empty((n, m.topology.classes), np.float32)
        hl = np.empty((n,), np.int32)
        hf = np.empty((n,), np.uint8)
        cnt = ctypes.c_int64(-1)
        _cabi.check(L.mdc_predict_host_checked(m._engine(), x.ctypes.data, n, hp.ctypes.data, hl.ctypes.data, hf.ctypes.data,
                                               ctypes.byref(cnt), _cabi.NONFINITE_PROPAGATE, chunk))
        np.testing.assert_array_equal(hp.view(np.int32), p.cpu().numpy().view(np.int32))
        np.testing.assert_array_equal(hl, l.cpu().numpy())
        np.testing.assert_array_equal(hf, f.cpu().numpy())
        assert cnt.value == len(bad)


def test_raise_names_exactly_the_bad_frames_and_default_is_unchanged():
    m = _model("deployed3", "f32")
    x, bad = _frames(5000, seed=3)
    for call in (lambda: m.predict(x, nonfinite="raise"), lambda: m.predict(torch.from_numpy(x).cuda(), nonfinite="raise"),
                 lambda: m.predict_classes(x, nonfinite="raise"), lambda: m.evaluate(x, np.zeros(5000, np.int64), nonfinite="raise")):
        with pytest.raises(NonFiniteInputError) as e:
            call()
        assert e.value.frames == bad and e.value.count == len(bad)
    clean = synthetic_frames(5000, seed=3)
    np.testing.assert_array_equal(m.predict(clean, nonfinite="raise").view(np.int32), m.predict(clean).view(np.int32))
    with pytest.raises(ValueError, match="tap"):
        m.forward_device(torch.from_numpy(clean).cuda(), tap="dense", nonfinite="propagate")
    # the default path is mdc_forward's: finite rows for the bad frames, as before this feature
    assert np.isfinite(m.predict(x)).all()


@pytest.mark.parametrize("topo,dtype", [("deployed3", "f32"), ("vtcnn2", "bf16"), ("cnnpy", "f32")])
def test_evaluate_propagates_nan_like_keras(topo, dtype):
    """cnn.py:153 prints nan when a test frame holds a NaN sample (the verdict's lost assertion of tests/test_eval_ops_gpu.py)."""
    m = _model(topo, dtype)
    clean = synthetic_frames(2000, seed=4)
    y = np.arange(2000) % m.topology.classes
    assert m.evaluate(clean, y, nonfinite="propagate") == pytest.approx(m.evaluate(clean, y), rel=1e-12)      # (f64 atomics: order only)
    dirty = clean.copy()
    dirty[1234, 1, 77] = np.nan
    assert np.isnan(m.evaluate(dirty, y, nonfinite="propagate"))
    assert np.isfinite(m.evaluate(dirty, y))          # (the default path, unchanged)


@pytest.mark.parametrize("topo,dtype", [("deployed10", "f32"), ("vtcnn2", "fp8"), ("cnnpy", "f32")])
def test_checked_forward_is_capturable(topo, dtype):
    m = _model(topo, dtype)
    n = 300
    dev = torch.device("cuda:0")
    x, _ = _frames(n)
    xd = torch.from_numpy(x).to(dev)
    probs = torch.empty((n, m.topology.classes), dtype=torch.float32, device=dev)
    labels = torch.empty((n,), dtype=torch.int32, device=dev)
    flags = torch.empty((n,), dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        m.forward_device(xd, probs, labels, nonfinite="propagate", nonfinite_out=flags)
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        m.forward_device(xd, probs, labels, nonfinite="propagate", nonfinite_out=flags)
    for seed in (6, 7):
        x2, _ = _frames(n, seed=seed)
        xd.copy_(torch.from_numpy(x2).to(dev))
        probs.zero_()
        labels.fill_(-1)
        flags.fill_(9)
        g.replay()
        torch.cuda.synchronize()
        fe = torch.empty_like(flags)
        pe, le, _ = m.forward_device(xd.clone(), nonfinite="propagate", nonfinite_out=fe)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_bits(probs), _bits(pe))
        assert torch.equal(labels, le) and torch.equal(flags, fe)


def test_zero_frames_and_bad_arguments_with_a_model():
    m = _model("deployed3", "f32")
    L = _cabi.lib()
    h = m._engine()
    assert L.mdc_forward_checked(h, None, 0, None, None, None, 0, None, None, 0, None) == 0
    xd = torch.zeros((4, 2, 128), device="cuda")
    assert L.mdc_forward_checked(h, xd.data_ptr(), 4, None, None, None, 0, None, None, 0, None) == -22
    assert L.mdc_forward_checked(h, xd.data_ptr(), 4, None, None, None, 0, xd.data_ptr(), None, 2, None) == -22
    flags = torch.full((4,), 9, dtype=torch.uint8, device="cuda")
    _cabi.check(L.mdc_forward_checked(h, xd.data_ptr(), 4, None, None, None, 0, flags.data_ptr(), None, 1, None))   # probs, labels, count: NULL
    torch.cuda.synchronize()
    assert flags.cpu().tolist() == [0, 0, 0, 0]
