"""mdc_iq_resample / frontend.resample / VTCNN2.predict_iq(interpolate=) on the MI355X.  The arithmetic is exact integers, so
every comparison is assert_array_equal (or torch.equal) against tests/iq_resample_ref.py (numpy int64, literal zero stuffing,
written from include/mdc.h):

  1. all three formats x (L, D, T) in SHAPES -- non-coprime L and D, odd and even D / g, branches of unequal length, empty branches
     (T < L: their outputs are exactly 0), the largest L, the largest D, the longest branch -- x P in {the largest without an
     output, the smallest with one, the smallest with two, 5 T / L + 3 D + 1, 40,001}; the base pointer one pair into a larger
     buffer; the output pre-filled with a sentinel, one guard pair after it untouched; the DDC test's captures (uniform with planted
     minimum, maximum and alternating runs); design_resampler taps and random-sign taps with every non-empty branch at
     sum |h| == 65535 exactly (a branch of one tap cannot reach that: its extreme is -32768); random phase0 and step.  At
     (32, 1, 1024) the 1.28 million outputs of P = 40,001 are held to the sparse reference at the tile seams, both ends and 400
     random places;
  2. L = 1 is mdc_iq_ddc: equal device tensors through both entry points;
  3. saturation at the documented phases and the phase steps {0, 1, 2^31, 2^32-1, a random odd one} at (5, 6, 48);
  4. pieces: the outputs of a prefix are a prefix; a call on the pairs from a on (a L = 0 mod D, phase0 + a step) gives the
     outputs from a L / D on -- a small a and one past the first tile;
  5. one run past grid cap x outputs per tile (the stride loop) at (2, 3, 4): first, last, the pass boundaries and 1,000 random
     outputs against the sparse reference, the whole output against a two-piece run;
  6. predict_iq(interpolate=5, decimate=6, shift=) == frontend.resample followed by predict_iq(out, "ci16"), bit for bit;
     interpolate=1 changes nothing;
  7. resample + mdc_iq_windows_norm + forward replay bit-identically from a captured graph;
  8. the example's synthetic capture, resampled by 6/5 and moved to +0.2 on the host (9.6 "samples per symbol"), classified with
     shift -0.2 / interpolate 5 / decimate 6, gives the squelch pattern and the window count of the original."""
import importlib.util
import math
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import iq_ddc_ref as DR                                                                  # noqa: E402
import iq_resample_ref as R                                                              # noqa: E402
from conftest import ROOT                                                                # noqa: E402
from test_iq_ddc_gpu import FORMATS, SENTINEL, _capture, _ddc, _extreme_taps, _net       # noqa: E402
from modulationdetectioncnn_amd import VTCNN2, _cabi, frontend                           # noqa: E402

SHAPES = [(1, 1, 1), (2, 1, 2), (2, 3, 5), (3, 2, 7), (4, 6, 24), (5, 6, 48), (5, 6, 47), (5, 6, 3), (32, 33, 264), (32, 1, 1024),
          (7, 128, 1024), (3, 256, 1024)]


def _first(T, L, D, outputs=1):
    """the smallest P with `outputs` outputs: (P - 1) L + 1 >= T + (outputs - 1) D"""
    return -(-(T + (outputs - 1) * D - 1) // L) + 1


def _tile_out(T, L, D):
    return (_cabi.RESAMPLE_TILE_PAIRS - -(-T // L)) // D * L


def _designed(L, D, T, seed=0):
    """design_resampler's taps; where every branch has at most one tap (T <= L) no design has unit gain in int16: random taps"""
    if T <= L:
        return np.random.default_rng(seed).integers(-32768, 32768, size=T).astype(np.int16)
    return frontend.design_resampler(L, D, ntaps=T)


def _extreme(L, T, seed):
    """random signs, every non-empty branch at sum |h| == 65535 exactly (one tap: -32768)"""
    h = np.zeros(T, np.int16)
    for r in range(min(L, T)):
        h[r::L] = _extreme_taps(len(range(r, T, L)), seed + r)
    sums = R.branch_abs_sums(h, L)
    assert all(s == 65535 or (s == 32768 and len(range(r, T, L)) == 1) or (s == 0 and r >= T) for r, s in enumerate(sums)), sums
    return h


def _resample(dev, fmt, pairs, phase0, step, L, D, h, guard=True):
    """mdc_iq_resample straight through the binding; dev: the device tensor whose data_ptr is pair 0.  Returns the (n_out, 2)
    device tensor after checking the guard pair."""
    lib = _cabi.lib()
    n_out = lib.mdc_iq_resample_out_count(pairs, h.size, L, D)
    assert n_out == R.out_count(pairs, h.size, L, D)
    out = torch.full((n_out + 1, 2), SENTINEL, dtype=torch.int16, device="cuda")
    _cabi.check(lib.mdc_iq_resample(dev.data_ptr(), R.FMT[fmt], pairs, phase0, step, L, D, h.ctypes.data, h.size, out.data_ptr(), n_out,
                                    torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    if guard:
        assert out[n_out].tolist() == [SENTINEL, SENTINEL]
    return out[:n_out]


# ---------------------------------------------------------------------------------------------------------------- 1. the grid of shapes
@pytest.mark.parametrize("L,D,T", SHAPES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_resample_is_the_reference(fmt, L, D, T):
    rng = np.random.default_rng(100000 * L + 1000 * D + T)
    for P in (_first(T, L, D) - 1, _first(T, L, D), _first(T, L, D, 2), 5 * T // L + 3 * D + 1, 40001):
        buf = _capture(fmt, P, seed=P + D)
        dev = torch.from_numpy(buf).cuda()[2:]                   # one pair into the allocation
        assert dev.data_ptr() % 256 == _cabi.IQ_PAIR_BYTES[R.FMT[fmt]]
        for h in (_designed(L, D, T, seed=P), _extreme(L, T, seed=P)):
            phase0, step = int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32))
            got = _resample(dev, fmt, P, phase0, step, L, D, h).cpu().numpy()
            n_out = R.out_count(P, T, L, D)
            assert got.shape == (n_out, 2)
            msg = f"{fmt} L {L} D {D} T {T} P {P} branch sums {R.branch_abs_sums(h, L)[:4]}"
            if n_out * T > 1 << 28:                              # (32, 1, 1024) at P = 40,001: the sparse reference
                tile = _tile_out(T, L, D)
                assert n_out > 4 * tile
                picks = np.unique(np.concatenate([np.arange(64), n_out - 1 - np.arange(64), rng.integers(0, n_out, size=400),
                                                  *[k * tile + np.arange(-2, 3) for k in range(1, n_out // tile + 1)]]))
                np.testing.assert_array_equal(got[picks], R.resample_sparse(buf[2:-2], fmt, phase0, step, L, D, h, picks.tolist()), err_msg=msg)
            else:
                np.testing.assert_array_equal(got, R.resample(buf[2:-2], fmt, phase0, step, L, D, h), err_msg=msg)
            if T < L and n_out:                                  # outputs of the empty branches r >= T: exactly 0
                r = (-np.arange(n_out) * D) % L
                assert ((r >= T).any() or n_out < L) and not got[r >= T].any(), msg


# ---------------------------------------------------------------------------------------------------------------- 2. L = 1 is the DDC
@pytest.mark.parametrize("D,T", [(1, 2), (3, 16), (12, 97), (64, 512)])
@pytest.mark.parametrize("fmt", FORMATS)
def test_one_branch_is_the_ddc(fmt, D, T):
    P = 30011
    buf = _capture(fmt, P, seed=D + T)
    dev = torch.from_numpy(buf).cuda()[2:]
    for h in (frontend.design_lowpass(max(D, 2), ntaps=T), _extreme_taps(T, seed=D)):
        phase0, step = 0x9E3779B9, frontend.phase_step(-0.2137)
        a = _resample(dev, fmt, P, phase0, step, 1, D, h)
        b = _ddc(dev, fmt, P, phase0, step, D, h)
        assert a.shape == b.shape == (DR.out_count(P, T, D), 2)
        assert torch.equal(a, b), (fmt, D, T)


# ---------------------------------------------------------------------------------------------------------------- 3. saturation, phase
def test_saturation_at_the_documented_phases():
    L, D, T = 5, 6, 48
    iq = np.full(2 * 300, -32768, np.dtype("<i2"))
    dev = torch.from_numpy(iq).cuda()
    unit = frontend.design_resampler(L, D, ntaps=T)              # every branch sums to 32768: DC gain exactly 1
    n = R.out_count(300, T, L, D)
    for phase0, want in ((5 << 29, (0, 32767)), (1 << 29, (0, -32768)), (0, (-32766, -32766))):      # (0, 32767): clamped from 46,340
        got = _resample(dev, "ci16", 300, phase0, 0, L, D, unit).cpu().numpy()
        np.testing.assert_array_equal(got, np.tile(np.array(want, np.int16), (n, 1)))
        np.testing.assert_array_equal(got, R.resample(iq, "ci16", phase0, 0, L, D, unit))
    h = _extreme(L, T, seed=3)
    for octant in range(8):
        got = _resample(dev, "ci16", 300, octant << 29, 0, L, D, h).cpu().numpy()
        np.testing.assert_array_equal(got, R.resample(iq, "ci16", octant << 29, 0, L, D, h))


@pytest.mark.parametrize("fmt", FORMATS)
def test_phase_steps(fmt):
    rng = np.random.default_rng(77)
    P, L, D, T = 9001, 5, 6, 48
    buf = _capture(fmt, P, seed=9)
    dev = torch.from_numpy(buf).cuda()[2:]
    h = frontend.design_resampler(L, D, ntaps=T)
    for step in (0, 1, 1 << 31, (1 << 32) - 1, int(rng.integers(0, 1 << 31)) * 2 + 1):
        phase0 = int(rng.integers(0, 1 << 32))
        got = _resample(dev, fmt, P, phase0, step, L, D, h).cpu().numpy()
        np.testing.assert_array_equal(got, R.resample(buf[2:-2], fmt, phase0, step, L, D, h), err_msg=f"step {step} phase0 {phase0}")


# ---------------------------------------------------------------------------------------------------------------- 4. pieces
@pytest.mark.parametrize("L,D,T", [(2, 3, 5), (5, 6, 48), (4, 6, 24), (32, 33, 264)])
@pytest.mark.parametrize("fmt", FORMATS)
def test_pieces(fmt, L, D, T):
    P = 30011
    buf = _capture(fmt, P, seed=L * D * T)
    dev = torch.from_numpy(buf).cuda()[2:]
    h = frontend.design_resampler(L, D, ntaps=T)
    phase0, step = 0x9E3779B9, frontend.phase_step(-0.2137)
    whole = _resample(dev, fmt, P, phase0, step, L, D, h)
    np.testing.assert_array_equal(whole.cpu().numpy(), R.resample(buf[2:-2], fmt, phase0, step, L, D, h))
    for P1 in (_first(T, L, D) + 5, 20001):                      # the outputs of a prefix are a prefix of the outputs
        part = _resample(dev, fmt, P1, phase0, step, L, D, h)
        assert 0 < part.shape[0] < whole.shape[0]
        assert torch.equal(part, whole[:part.shape[0]]), (fmt, L, D, T, P1)
    unit = D // math.gcd(L, D)                                   # a L = 0 (mod D)  <=>  a is a multiple of D / gcd(L, D)
    for a in (7 * unit, -(-9000 // unit) * unit):                # a tile reads at most 8192 pairs: the second a lies past the first
        j0 = a * L // D
        assert a * L % D == 0 and 0 < j0 < whole.shape[0]
        rest = _resample(dev[2 * a:], fmt, P - a, (phase0 + a * step) % (1 << 32), step, L, D, h)
        assert rest.shape[0] == whole.shape[0] - j0
        assert torch.equal(rest, whole[j0:]), (fmt, L, D, T, a)


# ---------------------------------------------------------------------------------------------------------------- 5. past the grid cap
def test_stride_loop_past_the_grid_cap():
    L, D, T, fmt = 2, 3, 4, "cu8"
    tile = _tile_out(T, L, D)
    cover = _cabi.RESAMPLE_GRID_CAP * tile                       # outputs one pass of the capped grid writes
    P = _first(T, L, D, 2 * cover + 3 * tile + 77)
    n_out = R.out_count(P, T, L, D)
    assert n_out >= 2 * cover + 3 * tile + 77
    g = torch.Generator(device="cuda").manual_seed(4)
    dev = torch.randint(0, 256, (2 * P,), dtype=torch.uint8, device="cuda", generator=g)
    iq = dev.cpu().numpy()
    h = np.array([20011, -12345, 7777, -30000], np.int16)        # two branches of two taps
    phase0, step = 0xC0FFEE11, 0x6789ABCD                        # an odd step
    whole = _resample(dev, fmt, P, phase0, step, L, D, h)
    assert whole.shape == (n_out, 2)
    rng = np.random.default_rng(8)
    picks = np.unique(np.concatenate([[0, n_out - 1, cover - 1, cover, 2 * cover - 1, 2 * cover], rng.integers(0, n_out, size=1000)]))
    np.testing.assert_array_equal(whole[torch.from_numpy(picks).cuda()].cpu().numpy(), R.resample_sparse(iq, fmt, phase0, step, L, D, h, picks.tolist()))
    a = 3 * (cover // 4 + 12345)                                 # off the tile grid: the second piece's tiles start elsewhere
    j0 = a * L // D
    first = _resample(dev, fmt, _first(T, L, D, j0), phase0, step, L, D, h)
    assert first.shape[0] == j0
    second = _resample(dev[2 * a:], fmt, P - a, (phase0 + a * step) % (1 << 32), step, L, D, h)
    assert torch.equal(torch.cat([first, second]), whole)


# ---------------------------------------------------------------------------------------------------------------- 6. predict_iq
def _wideband(fmt, pairs, seed):
    """The DDC test's wideband capture for a given length: a tone at +0.2 with a block-wise amplitude (powers spread over tens of
    dB), over a little noise and a DC offset."""
    rng = np.random.default_rng(seed)
    t = np.arange(pairs)
    full = {"cu8": 127.5, "ci8": 128.0, "ci16": 32768.0}[fmt]
    amp = np.repeat(rng.choice([0.002, 0.01, 0.05, 0.2, 0.7], size=pairs // 154 + 1), 154)[:pairs] * full
    z = amp * np.exp(2j * np.pi * (0.2 * t + 0.013 * np.sin(t / 50.0))) + 0.003 * full * (rng.standard_normal(pairs) + 1j * rng.standard_normal(pairs))
    mid = 127.5 if fmt == "cu8" else 0.0
    v = np.stack([z.real + mid + 0.01 * full, z.imag + mid - 0.02 * full], axis=1)
    return np.clip(np.rint(v), R.SAMPLE_MIN[fmt], R.SAMPLE_MAX[fmt]).astype(R.DTYPE[fmt]).reshape(-1)


def _pairs_for(windows, L, D, T):
    P = _first(T, L, D, 128 * windows)
    assert R.out_count(P, T, L, D) == 128 * windows
    return P


@pytest.mark.parametrize("name", ["deployed", "vtcnn2"])
def test_predict_iq_with_interpolate_is_resample_then_predict_iq(name):
    m = _net(name)
    L, D, windows = 5, 6, 64
    taps = frontend.design_resampler(L, D)
    for fmt in ("cu8", "ci16"):
        iq = _wideband(fmt, _pairs_for(windows, L, D, taps.size), seed=5)
        dev = torch.from_numpy(iq).cuda()
        kw = dict(normalize="rms", squelch_dbfs=-30.0, return_power=True)
        down = frontend.resample(dev, fmt, shift=-0.2, interpolate=L, decimate=D)
        assert down.shape == (128 * windows, 2) and down.dtype == torch.int16
        np.testing.assert_array_equal(down.cpu().numpy(), R.resample(iq, fmt, 0, frontend.phase_step(-0.2), L, D, taps))
        assert torch.equal(down, frontend.resample(dev, fmt, shift=-0.2, interpolate=2 * L, decimate=2 * D))      # reduced by the gcd
        p0, l0, w0 = m.predict_iq(down, "ci16", **kw)
        assert 0 < int((l0 < 0).sum()) < windows                 # the squelch separates something
        p1, l1, w1 = m.predict_iq(dev, fmt, shift=-0.2, interpolate=L, decimate=D, **kw)
        assert torch.equal(p0, p1) and torch.equal(l0, l1) and torch.equal(w0, w1)
        p2, l2, w2 = m.predict_iq(iq, fmt, shift=-0.2, interpolate=L, decimate=D, **kw)              # numpy in, numpy out
        assert isinstance(p2, np.ndarray) and isinstance(l2, np.ndarray) and isinstance(w2, np.ndarray)
        np.testing.assert_array_equal(p2.view(np.uint32), p0.cpu().numpy().view(np.uint32))
        np.testing.assert_array_equal(l2, l0.cpu().numpy())
        np.testing.assert_array_equal(w2, w0.cpu().numpy())
        # explicit taps, another hop, the plain (scaled) path
        other = frontend.design_resampler(L, D, ntaps=37)
        down = frontend.resample(dev, fmt, shift=0.1, interpolate=L, decimate=D, taps=other)
        pa, la = m.predict_iq(down, "ci16", 1.0 / 32768.0, hop=50)
        pb, lb = m.predict_iq(dev, fmt, hop=50, shift=0.1, interpolate=L, decimate=D, taps=other)
        assert torch.equal(pa, pb) and torch.equal(la, lb)
        # interpolate=1 is the call without the argument: the down-converter's route, and the plain one
        wide = _wideband(fmt, (128 * 8 - 1) * 12 + 96, seed=6)
        for src in (torch.from_numpy(wide).cuda(), wide):
            for args in (dict(shift=-0.2, decimate=12), dict(hop=64)):
                a = m.predict_iq(src, fmt, **args, **kw)
                b = m.predict_iq(src, fmt, interpolate=1, **args, **kw)
                for u, v in zip(a, b):
                    if isinstance(u, torch.Tensor):
                        assert torch.equal(u, v)
                    else:
                        np.testing.assert_array_equal(u, v)
    m._release()


# ---------------------------------------------------------------------------------------------------------------- 7. graph capture
def test_resample_norm_and_forward_are_capturable():
    L, D, windows, fmt = 5, 6, 48, "cu8"
    m = _net("vtcnn2")
    P = _pairs_for(windows, L, D, 8 * D)
    dev = torch.from_numpy(_wideband(fmt, P, seed=1)).cuda()
    kw = dict(normalize="rms", return_power=True, shift=-0.2, interpolate=L, decimate=D)
    m.predict_iq(dev, fmt, **kw)                                  # warm: workspace, code objects
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        p1, l1, w1 = m.predict_iq(dev, fmt, **kw)
    for seed in (2, 3):
        dev.copy_(torch.from_numpy(_wideband(fmt, P, seed=seed)).cuda())      # same buffer, new capture
        p1.zero_()
        l1.fill_(-5)
        g.replay()
        torch.cuda.synchronize()
        pe, le, we = m.predict_iq(dev, fmt, **kw)
        torch.cuda.synchronize()
        assert torch.equal(p1, pe) and torch.equal(l1, le) and torch.equal(w1, we), seed
    m._release()


# ---------------------------------------------------------------------------------------------------------------- 8. the example
def test_example_scenario_survives_a_symbol_rate_mismatch():
    """The example's synthetic capture (bursts at three gains, silence between them) is resampled by 6/5 on the host, in float
    (zero stuffing by 6, low-pass, every fifth sample), moved to +0.2 cycles per sample, given a tuner's DC offset and quantised
    to bytes again: it now arrives at 9.6 "samples per symbol".  classify(shift=-0.2, interpolate=5, decimate=6) must give as many
    windows as the original capture and squelch the same ones.  The two filters delay the stream by 47 samples at six times the
    original rate (under 8 original samples), so only the windows on either side of a burst edge may differ.  (The tuner's DC
    offset, 1.25 bytes, lands at -0.2 after the shift: INSIDE a 5/6 resampler's passband, unlike the DDC's.  The silent windows
    therefore sit near -39 dBFS instead of -45, still 4 dB under the squelch; the weakest burst is at -30.)"""
    spec = importlib.util.spec_from_file_location("classify_capture", os.path.join(ROOT, "examples", "classify_capture.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    orig = ex.synthetic_capture("cu8")
    z = (orig.astype(np.float64) - 127.5).reshape(-1, 2)
    z = z[:, 0] + 1j * z[:, 1]
    up = np.zeros(z.size * 6, complex)
    up[::6] = 6 * z
    up = np.convolve(up, frontend.design_lowpass(6).astype(np.float64) / 32768.0)[::5]      # "full": 47 samples longer, then 1 in 5
    up *= np.exp(2j * np.pi * 0.2 * np.arange(up.size))
    wide = np.clip(np.rint(np.stack([up.real + 128.6, up.imag + 126.9], axis=1)), 0, 255).astype(np.uint8).reshape(-1)
    model = VTCNN2.synthetic("deployed3")
    _, l_orig, pw_orig = ex.classify(model, orig, "cu8")
    _, l_wide, pw_wide = ex.classify(model, wide, "cu8", shift=-0.2, interpolate=5, decimate=6)
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
