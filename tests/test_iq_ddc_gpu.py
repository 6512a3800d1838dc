"""mdc_iq_ddc / frontend.ddc / VTCNN2.predict_iq(shift=, decimate=) on the MI355X.  The arithmetic is exact integers, so every
comparison is assert_array_equal against tests/iq_ddc_ref.py (numpy int64, written from include/mdc.h):

  1. all three formats x (D, T) in {(1,1), (1,2), (2,5), (3,16), (12,96), (12,97), (64,512), (256,1024)} x P in {T-1, T, T+D-1,
     T+D, 5T+3D+1, 40,001}: odd j D (the output's first sample in the high half of a dword), odd T, tiles at the capture's end,
     more than one tile; the base pointer one pair into a larger buffer (2-byte alignment for the 8-bit formats); the output
     pre-filled with a sentinel, one guard pair after it untouched; inputs uniform over the full range with planted runs of
     all-minimum, all-maximum and alternating minimum / maximum pairs; design_lowpass taps and random-sign taps with
     sum |h| == 65535 exactly (T = 1 cannot reach that: its extreme is the single tap -32768);
  2. saturation and phase: all-minimum CI16 at phase_step 0 clamps as documented; steps {0, 1, 2^31, 2^32-1, a random odd value}
     with random phase0;
  3. seam identity: a capture processed in two calls -- the second from pair a = 7 D (and from a later multiple of D) with
     phase0 + a step, the pieces overlapping by T - D pairs -- equals the single call;
  4. one run past grid cap x outputs per tile (the stride loop): first, last and 1,000 random outputs against the reference,
     and the whole output against a two-piece run split off the tile grid;
  5. predict_iq(shift=, decimate=) == frontend.ddc followed by predict_iq(out, "ci16"), bit for bit, probabilities, labels and
     power, for a deployed net and VT-CNN2, tensor and numpy input; the default arguments change nothing;
  6. ddc + mdc_iq_windows_norm + forward replay bit-identically from a captured graph;
  7. examples/classify_capture.py's scenario: its synthetic capture interpolated by 12 and moved to +0.2 cycles per sample on
     the host gives, classified with shift -0.2 / decimate 12, the squelch pattern of the original capture."""
import importlib.util
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import iq_ddc_ref as R                                                                   # noqa: E402
from conftest import GOLDEN, ROOT                                                        # noqa: E402
from modulationdetectioncnn_amd import VTCNN2, Topology, _cabi, frontend                 # noqa: E402

FORMATS = ["cu8", "ci8", "ci16"]
TORCH_DTYPE = {"cu8": torch.uint8, "ci8": torch.int8, "ci16": torch.int16}
SHAPES = [(1, 1), (1, 2), (2, 5), (3, 16), (12, 96), (12, 97), (64, 512), (256, 1024)]
SENTINEL = 0x5A5A


def _capture(fmt, pairs, seed):
    """One pair of padding + `pairs` pairs + one pair of padding (so that even an empty capture has an address): uniform over the whole range, with runs of 300 pairs of all minimum, all maximum and
    alternating minimum / maximum pairs (cut off where the capture is shorter)."""
    lo, hi, dt = R.SAMPLE_MIN[fmt], R.SAMPLE_MAX[fmt], R.DTYPE[fmt]
    buf = np.random.default_rng(seed).integers(lo, hi + 1, size=2 * (pairs + 2)).astype(dt)
    body = buf[2:-2]
    alt = np.empty(600, dt)
    alt[0::4], alt[1::4], alt[2::4], alt[3::4] = lo, lo, hi, hi
    for at, run in ((0, np.full(600, lo, dt)), (700, np.full(600, hi, dt)), (1500, alt), (max(0, pairs - 200), np.full(600, lo, dt))):
        seg = body[2 * at: 2 * at + 600]
        seg[:] = run[:seg.size]
    return buf


def _lowpass(D, T):
    if T == 1:
        return np.array([32767], np.int16)                       # (one tap cannot hold 32768)
    return frontend.design_lowpass(max(D, 2), ntaps=T)


def _extreme_taps(T, seed):
    """random signs, sum |h| == 65535 exactly"""
    rng = np.random.default_rng(seed)
    if T == 1:
        return np.array([-32768], np.int16)
    if T == 2:
        return np.array([32767, -32768], np.int16)
    w = rng.uniform(0.2, 1.0, size=T)
    a = np.minimum(np.floor(w / w.sum() * 65535).astype(np.int64), 32767)
    k = 0
    while a.sum() < 65535:                                       # hand out what the rounding left
        if a[k % T] < 32767:
            a[k % T] += min(32767 - a[k % T], 65535 - a.sum())
        k += 1
    h = a * rng.choice([-1, 1], size=T)
    assert int(np.abs(h).sum()) == 65535 and h.min() >= -32768 and h.max() <= 32767
    return h.astype(np.int16)


def _ddc(dev, fmt, pairs, phase0, step, D, h, guard=True):
    """mdc_iq_ddc straight through the binding; dev: the device tensor whose data_ptr is pair 0.  Returns the (n_out, 2) device
    tensor after checking the guard pair."""
    L = _cabi.lib()
    n_out = L.mdc_iq_ddc_out_count(pairs, h.size, D)
    assert n_out == R.out_count(pairs, h.size, D)
    out = torch.full((n_out + 1, 2), SENTINEL, dtype=torch.int16, device="cuda")
    _cabi.check(L.mdc_iq_ddc(dev.data_ptr(), R.FMT[fmt], pairs, phase0, step, D, h.ctypes.data, h.size, out.data_ptr(), n_out,
                             torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    if guard:
        assert out[n_out].tolist() == [SENTINEL, SENTINEL]
    return out[:n_out]


# ---------------------------------------------------------------------------------------------------------------- 1. the grid of shapes
@pytest.mark.parametrize("D,T", SHAPES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_ddc_is_the_reference(fmt, D, T):
    rng = np.random.default_rng(1000 * D + T)
    for P in (T - 1, T, T + D - 1, T + D, 5 * T + 3 * D + 1, 40001):
        buf = _capture(fmt, P, seed=P + D)
        dev = torch.from_numpy(buf).cuda()[2:]                   # one pair into the allocation
        assert dev.data_ptr() % 256 == _cabi.IQ_PAIR_BYTES[R.FMT[fmt]]
        for h in (_lowpass(D, T), _extreme_taps(T, seed=P)):
            phase0, step = int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32))
            got = _ddc(dev, fmt, P, phase0, step, D, h).cpu().numpy()
            want = R.ddc(buf[2:-2], fmt, phase0, step, D, h)
            assert got.shape == want.shape == (R.out_count(P, T, D), 2)
            np.testing.assert_array_equal(got, want, err_msg=f"{fmt} D {D} T {T} P {P} sum|h| {int(np.abs(h.astype(np.int64)).sum())}")


# ---------------------------------------------------------------------------------------------------------------- 2. saturation, phase
def test_saturation_at_the_documented_phases():
    iq = np.full(2 * 300, -32768, np.dtype("<i2"))
    dev = torch.from_numpy(iq).cuda()
    unit = np.array([16384, 16384], np.int16)                    # DC gain exactly 1
    for phase0, want in ((5 << 29, (0, 32767)), (1 << 29, (0, -32768)), (0, (-32766, -32766))):      # (0, 32767): clamped from 46,340
        got = _ddc(dev, "ci16", 300, phase0, 0, 1, unit).cpu().numpy()
        np.testing.assert_array_equal(got, np.tile(np.array(want, np.int16), (299, 1)))
        np.testing.assert_array_equal(got, R.ddc(iq, "ci16", phase0, 0, 1, unit))
    for h in (frontend.design_lowpass(3), _extreme_taps(24, seed=3)):       # the same through real filters, every octant
        for octant in range(8):
            got = _ddc(dev, "ci16", 300, octant << 29, 0, 3, h).cpu().numpy()
            np.testing.assert_array_equal(got, R.ddc(iq, "ci16", octant << 29, 0, 3, h))


@pytest.mark.parametrize("fmt", FORMATS)
def test_phase_steps(fmt):
    rng = np.random.default_rng(77)
    P, D = 9001, 3
    buf = _capture(fmt, P, seed=9)
    dev = torch.from_numpy(buf).cuda()[2:]
    h = frontend.design_lowpass(D, ntaps=16)
    for step in (0, 1, 1 << 31, (1 << 32) - 1, int(rng.integers(0, 1 << 31)) * 2 + 1):
        phase0 = int(rng.integers(0, 1 << 32))
        got = _ddc(dev, fmt, P, phase0, step, D, h).cpu().numpy()
        np.testing.assert_array_equal(got, R.ddc(buf[2:-2], fmt, phase0, step, D, h), err_msg=f"step {step} phase0 {phase0}")


# ---------------------------------------------------------------------------------------------------------------- 3. seams
def _two_pieces(dev, fmt, P, phase0, step, D, h, a):
    """outputs of pairs [0, a + T - D) then of pairs [a, P), the second with the oscillator where the single call has it"""
    pb = 2          # samples per pair in the flat tensor
    first = _ddc(dev, fmt, a + h.size - D, phase0, step, D, h, guard=True)
    second = _ddc(dev[pb * a:], fmt, P - a, (phase0 + a * step) % (1 << 32), step, D, h, guard=True)
    return torch.cat([first, second])


@pytest.mark.parametrize("D,T", [(2, 5), (3, 16), (12, 96), (12, 97)])
@pytest.mark.parametrize("fmt", FORMATS)
def test_seam_identity(fmt, D, T):
    P = 30011
    buf = _capture(fmt, P, seed=D * T)
    dev = torch.from_numpy(buf).cuda()[2:]
    h = _lowpass(D, T)
    phase0, step = 0x9E3779B9, frontend.phase_step(-0.2137)
    whole = _ddc(dev, fmt, P, phase0, step, D, h)
    np.testing.assert_array_equal(whole.cpu().numpy(), R.ddc(buf[2:-2], fmt, phase0, step, D, h))
    for a in (7 * D, 1001 * D):
        pieces = _two_pieces(dev, fmt, P, phase0, step, D, h, a)
        assert pieces.shape == whole.shape
        assert torch.equal(pieces, whole), (fmt, D, T, a)


# ---------------------------------------------------------------------------------------------------------------- 4. past the grid cap
def test_stride_loop_past_the_grid_cap():
    D, T, fmt = 2, 2, "cu8"
    tile_out = (_cabi.DDC_TILE_PAIRS - T) // D + 1
    cover = _cabi.DDC_GRID_CAP * tile_out                        # outputs one pass of the capped grid writes
    n_out = 2 * cover + 3 * tile_out + 77
    P = (n_out - 1) * D + T
    g = torch.Generator(device="cuda").manual_seed(4)
    dev = torch.randint(0, 256, (2 * P,), dtype=torch.uint8, device="cuda", generator=g)
    iq = dev.cpu().numpy()
    h = np.array([20011, -12345], np.int16)
    phase0, step = 0xC0FFEE11, 0x6789ABCD                        # an odd step
    whole = _ddc(dev, fmt, P, phase0, step, D, h)
    assert whole.shape == (n_out, 2)
    rng = np.random.default_rng(8)
    picks = np.unique(np.concatenate([[0, n_out - 1, cover - 1, cover, 2 * cover - 1, 2 * cover], rng.integers(0, n_out, size=1000)]))
    np.testing.assert_array_equal(whole[torch.from_numpy(picks).cuda()].cpu().numpy(), R.ddc_sparse(iq, fmt, phase0, step, D, h, picks.tolist()))
    a = D * (cover // 2 + 12345)                                 # off the tile grid: the second piece's tiles start elsewhere
    assert torch.equal(_two_pieces(dev, fmt, P, phase0, step, D, h, a), whole)


# ---------------------------------------------------------------------------------------------------------------- 5. predict_iq
def _net(name):
    if name == "deployed":
        return VTCNN2.from_npz(os.path.join(GOLDEN, "weights", "3convmodrecnets_CNN2_0.5.npz"))
    return VTCNN2.synthetic(Topology.vtcnn2(11), seed=2016, dtype="bf16")


def _wideband(fmt, windows, D, seed):
    """A capture whose decimated stream holds `windows` disjoint windows with powers spread over tens of dB: a tone at +0.2 with
    a block-wise amplitude, over a little noise and a DC offset."""
    rng = np.random.default_rng(seed)
    P = (128 * windows - 1) * D + 8 * D
    t = np.arange(P)
    full = {"cu8": 127.5, "ci8": 128.0, "ci16": 32768.0}[fmt]
    amp = np.repeat(rng.choice([0.002, 0.01, 0.05, 0.2, 0.7], size=P // (128 * D) + 1), 128 * D)[:P] * full
    z = amp * np.exp(2j * np.pi * (0.2 * t + 0.013 * np.sin(t / 50.0))) + 0.003 * full * (rng.standard_normal(P) + 1j * rng.standard_normal(P))
    mid = 127.5 if fmt == "cu8" else 0.0
    v = np.stack([z.real + mid + 0.01 * full, z.imag + mid - 0.02 * full], axis=1)
    return np.clip(np.rint(v), R.SAMPLE_MIN[fmt], R.SAMPLE_MAX[fmt]).astype(R.DTYPE[fmt]).reshape(-1)


@pytest.mark.parametrize("name", ["deployed", "vtcnn2"])
def test_predict_iq_with_ddc_is_ddc_then_predict_iq(name):
    m = _net(name)
    D, windows = 12, 64
    for fmt in ("cu8", "ci16"):
        iq = _wideband(fmt, windows, D, seed=5)
        dev = torch.from_numpy(iq).cuda()
        kw = dict(normalize="rms", squelch_dbfs=-30.0, return_power=True)
        down = frontend.ddc(dev, fmt, shift=-0.2, decimate=D)
        assert down.shape == (128 * windows, 2) and down.dtype == torch.int16
        np.testing.assert_array_equal(down.cpu().numpy(), R.ddc(iq, fmt, 0, frontend.phase_step(-0.2), D, frontend.design_lowpass(D)))
        p0, l0, w0 = m.predict_iq(down, "ci16", **kw)
        assert 0 < int((l0 < 0).sum()) < windows                 # the squelch separates something
        p1, l1, w1 = m.predict_iq(dev, fmt, shift=-0.2, decimate=D, **kw)
        assert torch.equal(p0, p1) and torch.equal(l0, l1) and torch.equal(w0, w1)
        p2, l2, w2 = m.predict_iq(iq, fmt, shift=-0.2, decimate=D, **kw)                     # numpy in, numpy out
        assert isinstance(p2, np.ndarray) and isinstance(l2, np.ndarray) and isinstance(w2, np.ndarray)
        np.testing.assert_array_equal(p2.view(np.uint32), p0.cpu().numpy().view(np.uint32))
        np.testing.assert_array_equal(l2, l0.cpu().numpy())
        np.testing.assert_array_equal(w2, w0.cpu().numpy())
        # explicit taps, another hop, the plain (scaled) path: scale=None means 1/32768
        taps = frontend.design_lowpass(D, ntaps=64)
        down = frontend.ddc(dev, fmt, shift=0.1, decimate=D, taps=taps)
        pa, la = m.predict_iq(down, "ci16", 1.0 / 32768.0, hop=50)
        pb, lb = m.predict_iq(dev, fmt, hop=50, shift=0.1, decimate=D, taps=taps)
        assert torch.equal(pa, pb) and torch.equal(la, lb)
        # the defaults change nothing
        for src in (dev, iq):
            a = m.predict_iq(src, fmt, hop=64, **kw)
            b = m.predict_iq(src, fmt, hop=64, shift=0.0, decimate=1, taps=None, **kw)
            for u, v in zip(a, b):
                if isinstance(u, torch.Tensor):
                    assert torch.equal(u, v)
                else:
                    np.testing.assert_array_equal(u, v)
    m._release()


# ---------------------------------------------------------------------------------------------------------------- 6. graph capture
def test_ddc_norm_and_forward_are_capturable():
    D, windows, fmt = 12, 48, "cu8"
    m = _net("vtcnn2")
    dev = torch.from_numpy(_wideband(fmt, windows, D, seed=1)).cuda()
    kw = dict(normalize="rms", return_power=True, shift=-0.2, decimate=D)
    m.predict_iq(dev, fmt, **kw)                                  # warm: workspace, code objects
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        p1, l1, w1 = m.predict_iq(dev, fmt, **kw)
    for seed in (2, 3):
        dev.copy_(torch.from_numpy(_wideband(fmt, windows, D, seed=seed)).cuda())      # same buffer, new capture
        p1.zero_()
        l1.fill_(-5)
        g.replay()
        torch.cuda.synchronize()
        pe, le, we = m.predict_iq(dev, fmt, **kw)
        torch.cuda.synchronize()
        assert torch.equal(p1, pe) and torch.equal(l1, le) and torch.equal(w1, we), seed
    m._release()


# ---------------------------------------------------------------------------------------------------------------- 7. the example
def test_example_scenario_survives_a_trip_through_a_wideband_capture():
    """The example's synthetic capture (bursts at three gains, silence between them) is interpolated by 12 (zero stuffing +
    low-pass, float, on the host), moved to +0.2 cycles per sample, given a tuner's DC offset and quantised to bytes again;
    classify(shift=-0.2, decimate=12) must squelch the windows the original capture's classification squelches.  The two
    filters delay the stream by 95 wideband samples (under 8 output samples), so only windows next to a burst edge may differ."""
    spec = importlib.util.spec_from_file_location("classify_capture", os.path.join(ROOT, "examples", "classify_capture.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    D = 12
    orig = ex.synthetic_capture("cu8")
    z = (orig.astype(np.float64) - 127.5).reshape(-1, 2)
    z = z[:, 0] + 1j * z[:, 1]
    up = np.zeros(z.size * D, complex)
    up[::D] = D * z
    up = np.convolve(up, frontend.design_lowpass(D).astype(np.float64) / 32768.0)           # "full": 95 samples longer
    up *= np.exp(2j * np.pi * 0.2 * np.arange(up.size))
    wide = np.clip(np.rint(np.stack([up.real + 128.6, up.imag + 126.9], axis=1)), 0, 255).astype(np.uint8).reshape(-1)
    model = VTCNN2.synthetic("deployed3")
    _, l_orig, pw_orig = ex.classify(model, orig, "cu8")
    _, l_wide, pw_wide = ex.classify(model, wide, "cu8", shift=-0.2, decimate=D)
    assert l_orig.shape == l_wide.shape == (z.size // 128,)
    sq_orig, sq_wide = l_orig < 0, l_wide < 0
    assert 0 < sq_orig.sum() < sq_orig.size
    edge = np.zeros(sq_orig.size, bool)
    change = np.flatnonzero(sq_orig[1:] != sq_orig[:-1]) + 1      # first window of each new stretch
    for c in change:
        edge[max(0, c - 1): c + 1] = True                         # the windows on either side of the edge
    print(f"{sq_orig.size} windows, {int(sq_orig.sum())} squelched, {int(edge.sum())} at burst edges; largest power difference off the edges "
          f"{np.abs(pw_orig - pw_wide)[~edge & ~sq_orig].max():.2f} dB")
    np.testing.assert_array_equal(sq_wide[~edge], sq_orig[~edge])
    model._release()
