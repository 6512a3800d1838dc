"""mdc_iq_spectrogram / frontend.spectrogram / VTCNN2.scan_iq on the MI355X, against tests/iq_spectrum_ref.py (float64 numpy,
written from include/mdc.h):

  1. parity: nfft in 64..4096 x the three formats x (hop, avg) in {(1, 1), (nfft/2, 3), (nfft, 1), (nfft+3, 2)} -- every pass
     structure of the mixed-radix transform, overlap, no overlap, skipped pairs -- on a capture just long enough for 5 rows, on
     pairs == nfft and on pairs == nfft - 1; the base pointer one pair into a larger allocation; the output pre-filled with a
     sentinel, one guard row after it untouched; inputs uniform over the full range with planted runs of all-minimum, all-maximum
     and alternating pairs, the later part two off-bin tones 40 dB apart; design_window and an asymmetric random window.  The
     tolerance is the header's, every term from the reference:
         |P^ - P| <= mean_s[2 eps sqrt(P_s[k] T_s) + eps^2 T_s] + (avg + 4) u P[r,k],  u = 2^-24, eps = 8u (log2 nfft + 1);
  2. the same call twice gives the same bits; row r of a 9-row call is, bit for bit, the one row of the sub-capture from r avg hop;
  3. past the grid cap: first, last, the rows around each multiple of the cap and 200 random rows against the reference, the whole
     output against a two-piece run split off the cap's grid;
  4. frontend.spectrogram with its cached window replays bit-identically from a captured graph after the input is overwritten;
  5. the scan end to end: device spectrum -> find_emitters gives the reference spectrum's three emitters; VTCNN2.scan_iq's plans,
     and its results against tuning, resampling and classifying by hand; the example's --scan path."""
import functools
import importlib.util
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import iq_spectrum_ref as S                                                              # noqa: E402
from conftest import GOLDEN, ROOT                                                        # noqa: E402
from modulationdetectioncnn_amd import VTCNN2, _cabi, frontend                           # noqa: E402

FORMATS = ["cu8", "ci8", "ci16"]
NFFTS = [64, 128, 256, 512, 1024, 2048, 4096]
SENTINEL = -7.0


def _capture(fmt, pairs, seed):
    """One pair of padding + `pairs` pairs + one pair of padding.  Uniform over the whole range; from the middle on two off-bin
    tones, 0.6 and 0.006 of full scale; runs of 300 pairs of all minimum, all maximum and alternating minimum / maximum pairs at
    pairs 0, 700, 1500 and 200 before the end (cut off where the capture is shorter)."""
    lo, hi, dt = S.SAMPLE_MIN[fmt], S.SAMPLE_MAX[fmt], S.DTYPE[fmt]
    rng = np.random.default_rng(seed)
    buf = rng.integers(lo, hi + 1, size=2 * (pairs + 2)).astype(dt)
    body = buf[2:2 + 2 * pairs]
    half = pairs // 2
    n = np.arange(half, pairs)
    z = 0.6 * np.exp(2j * np.pi * (0.1234567 * n + 0.3)) + 0.006 * np.exp(-2j * np.pi * (0.3141593 * n + 0.1))
    mid, amp = (lo + hi) / 2.0, (hi - lo) / 2.0
    body[2 * half:] = np.clip(np.rint(np.stack([z.real, z.imag], axis=1) * amp + mid), lo, hi).astype(dt).reshape(-1)
    alt = np.empty(600, dt)
    alt[0::4], alt[1::4], alt[2::4], alt[3::4] = lo, lo, hi, hi
    for at, run in ((0, np.full(600, lo, dt)), (700, np.full(600, hi, dt)), (1500, alt), (max(0, pairs - 200), np.full(600, lo, dt))):
        seg = body[2 * at: 2 * at + 600]
        seg[:] = run[:seg.size]
    return buf


def _random_window(nfft, seed):
    return np.random.default_rng(seed).integers(0, 32768, size=nfft).astype(np.int16)      # asymmetric: a reversed or shifted index shows


def _spectrogram(dev, fmt, pairs, nfft, hop, avg, wdev, scale):
    """mdc_iq_spectrogram straight through the binding; dev: the device tensor whose data_ptr is pair 0.  Returns the (rows, nfft)
    device tensor after checking the guard row."""
    L = _cabi.lib()
    rows = L.mdc_iq_spectrogram_rows(pairs, nfft, hop, avg)
    assert rows == S.rows_count(pairs, nfft, hop, avg)
    out = torch.full((rows + 1, nfft), SENTINEL, dtype=torch.float32, device="cuda")
    _cabi.check(L.mdc_iq_spectrogram(dev.data_ptr(), S.FMT[fmt], pairs, nfft, hop, avg, wdev.data_ptr(), scale, out.data_ptr(), rows,
                                     torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert bool((out[rows] == SENTINEL).all())
    return out[:rows]


def _worst_ratio(got, iq, fmt, nfft, hop, avg, w, scale, rows=None):
    """largest |got - P| / bound over the rows (all, or the listed ones), every term of the bound from the float64 reference"""
    P, Ps, Ts = S.spectrogram(iq, fmt, nfft, hop, avg, w, scale, rows)
    assert got.shape == P.shape
    if P.size == 0:
        return 0.0
    assert np.all(np.isfinite(got)) and got.min() >= 0.0                                   # in particular no sentinel is left
    return float((np.abs(got.astype(np.float64) - P) / S.bound(P, Ps, Ts, nfft, avg)).max())


# ---------------------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("nfft", NFFTS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_spectrogram_is_the_reference(fmt, nfft):
    worst = 0.0
    windows = [frontend.design_window(nfft), _random_window(nfft, seed=nfft)]
    for hop, avg in ((1, 1), (nfft // 2, 3), (nfft, 1), (nfft + 3, 2)):
        for pairs in (nfft + (5 * avg - 1) * hop, nfft, nfft - 1):
            buf = _capture(fmt, pairs, seed=nfft + hop + pairs)
            dev = torch.from_numpy(buf).cuda()[2:]                   # one pair into the allocation
            assert dev.data_ptr() % 256 == _cabi.IQ_PAIR_BYTES[S.FMT[fmt]]
            for w in windows:
                scale = frontend.window_scale(w)
                got = _spectrogram(dev, fmt, pairs, nfft, hop, avg, torch.from_numpy(w).cuda(), scale).cpu().numpy()
                assert got.shape == (5 if pairs > nfft else 1 if pairs == nfft and avg == 1 else 0, nfft)
                ratio = _worst_ratio(got, buf[2:2 + 2 * pairs], fmt, nfft, hop, avg, w, scale)
                worst = max(worst, ratio)
                assert ratio <= 1.0, (fmt, nfft, hop, avg, pairs, ratio)
    print(f"{fmt} nfft {nfft}: largest error / bound {worst:.4f}")


# ---------------------------------------------------------------------------------------------------------------- 2. determinism, seams
@pytest.mark.parametrize("nfft", [256, 4096])
@pytest.mark.parametrize("fmt", FORMATS)
def test_determinism_and_seam_identity(fmt, nfft):
    hop, avg, rows = nfft // 2 + 1, 3, 9
    pairs = nfft + (rows * avg - 1) * hop
    buf = _capture(fmt, pairs, seed=nfft)
    dev = torch.from_numpy(buf).cuda()[2:]
    w = _random_window(nfft, seed=3)
    wdev, scale = torch.from_numpy(w).cuda(), frontend.window_scale(w)
    whole = _spectrogram(dev, fmt, pairs, nfft, hop, avg, wdev, scale)
    assert whole.shape == (rows, nfft)
    assert torch.equal(whole, _spectrogram(dev, fmt, pairs, nfft, hop, avg, wdev, scale))
    assert _worst_ratio(whole.cpu().numpy(), buf[2:2 + 2 * pairs], fmt, nfft, hop, avg, w, scale) <= 1.0
    one = nfft + (avg - 1) * hop                                 # pairs of exactly one row
    for r in range(rows):
        piece = _spectrogram(dev[2 * r * avg * hop:], fmt, one, nfft, hop, avg, wdev, scale)
        assert piece.shape == (1, nfft) and torch.equal(piece[0], whole[r]), (fmt, nfft, r)


# ---------------------------------------------------------------------------------------------------------------- 3. past the grid cap
def test_stride_loop_past_the_grid_cap():
    nfft, hop, avg, fmt = 64, 64, 1, "cu8"
    cap = _cabi.SPECTROGRAM_GRID_CAP
    rows = 2 * cap + 5
    pairs = nfft + (rows - 1) * hop
    g = torch.Generator(device="cuda").manual_seed(4)
    dev = torch.randint(0, 256, (2 * pairs,), dtype=torch.uint8, device="cuda", generator=g)
    iq = dev.cpu().numpy()
    w = _random_window(nfft, seed=9)
    wdev, scale = torch.from_numpy(w).cuda(), frontend.window_scale(w)
    whole = _spectrogram(dev, fmt, pairs, nfft, hop, avg, wdev, scale)
    assert whole.shape == (rows, nfft)
    rng = np.random.default_rng(8)
    picks = np.unique(np.concatenate([[0, rows - 1, cap - 1, cap, 2 * cap - 1, 2 * cap], rng.integers(0, rows, size=200)]))
    ratio = _worst_ratio(whole[torch.from_numpy(picks).cuda()].cpu().numpy(), iq, fmt, nfft, hop, avg, w, scale, rows=picks)
    print(f"largest error / bound {ratio:.4f}")
    assert ratio <= 1.0
    a = cap // 2 + 123                                           # rows of the first piece: the second piece's grid starts off the cap's
    first = _spectrogram(dev, fmt, a * hop, nfft, hop, avg, wdev, scale)
    second = _spectrogram(dev[2 * a * hop:], fmt, pairs - a * hop, nfft, hop, avg, wdev, scale)
    assert first.shape[0] == a and torch.equal(torch.cat([first, second]), whole)


# ---------------------------------------------------------------------------------------------------------------- 4. graph capture
def test_spectrogram_is_capturable():
    nfft, avg, fmt = 1024, 2, "ci16"
    pairs = nfft + 11 * (nfft // 2)
    dev = torch.from_numpy(_capture(fmt, pairs, seed=1)[2:-2].copy()).cuda()
    frontend.spectrogram(dev, fmt, nfft=nfft, avg=avg)            # warm: the cached window, code objects
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        p1 = frontend.spectrogram(dev, fmt, nfft=nfft, avg=avg)
    assert p1.shape == (6, nfft)
    for seed in (2, 3):
        dev.copy_(torch.from_numpy(_capture(fmt, pairs, seed=seed)[2:-2].copy()).cuda())      # same buffer, new capture
        p1.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        pe = frontend.spectrogram(dev, fmt, nfft=nfft, avg=avg)
        torch.cuda.synchronize()
        assert torch.equal(p1, pe) and float(pe.min()) >= 0.0, seed


# ---------------------------------------------------------------------------------------------------------------- 5. end to end
@functools.lru_cache(maxsize=None)
def _band():
    return S.synthetic_band(1)                                   # shared: nobody writes to it


def test_device_spectrum_finds_the_reference_emitters():
    nfft, iq = 1024, _band()
    w = frontend.design_window(nfft)
    want = frontend.find_emitters(S.band_psd(iq, nfft, w, frontend.window_scale(w)), window=w)
    spec = frontend.spectrogram(iq, "ci16", nfft=nfft)            # hop nfft/2, avg 1: the reference spectrum's segments
    assert spec.shape == (S.rows_count(iq.size // 2, nfft, nfft // 2, 1), nfft)
    got = frontend.find_emitters(spec.to(torch.float64).mean(0).cpu(), window=w)
    assert len(got) == len(want) == 3
    for a, b in zip(got, want):
        assert abs(a.centre - b.centre) <= 1.0 / nfft and abs(a.bandwidth - b.bandwidth) <= 1.0 / nfft
        assert abs(a.power_dbfs - b.power_dbfs) < 0.01 and abs(a.snr_db - b.snr_db) < 0.01


def test_scan_iq_is_spectrogram_plan_resample_and_predict_by_hand():
    nfft, avg, iq = 1024, 8, _band()
    m = VTCNN2.from_npz(os.path.join(GOLDEN, "weights", "3convmodrecnets_CNN2_0.5.npz"))
    dev = torch.from_numpy(iq.copy()).cuda()
    records = m.scan_iq(dev, "ci16", nfft=nfft, avg=avg, squelch_dbfs=-60.0)
    w = frontend.design_window(nfft)
    emitters = frontend.find_emitters(frontend.spectrogram(dev, "ci16", nfft=nfft, avg=avg).to(torch.float64).mean(0).cpu(), window=w)
    assert len(records) == len(emitters) == 3
    for rec, e, fc in zip(records, emitters, S.BAND_CENTRES):
        shift, L, D, _ = frontend.channel_plan(e.centre, e.bandwidth)
        assert (rec["centre"], rec["bandwidth"], rec["power_dbfs"], rec["snr_db"]) == tuple(e) and abs(e.centre - fc) < 0.001
        assert (rec["shift"], rec["interpolate"], rec["decimate"]) == (shift, L, D)
        taps = frontend.plan_taps(L, D)
        down = frontend.ddc(dev, "ci16", shift=shift, decimate=D, taps=taps) if L == 1 else \
            frontend.resample(dev, "ci16", shift=shift, interpolate=L, decimate=D, taps=taps)
        down = down[:down.shape[0] // 128 * 128]
        assert down.shape[0] >= 128
        p, l, d = m.predict_iq(down.reshape(-1), "ci16", normalize="rms", squelch_dbfs=-60.0, return_power=True)
        assert torch.equal(rec["probs"], p) and torch.equal(rec["labels"], l) and torch.equal(rec["window_dbfs"], d)
        open_ = l[l >= 0]
        assert open_.numel() > 0 and rec["label"] == int(torch.bincount(open_).argmax())
    by_numpy = m.scan_iq(iq, "ci16", nfft=nfft, avg=avg, squelch_dbfs=-60.0)             # numpy in, numpy out
    for rec, ref in zip(by_numpy, records):
        assert isinstance(rec["probs"], np.ndarray) and rec["label"] == ref["label"] and rec["decimate"] == ref["decimate"]
        np.testing.assert_array_equal(rec["probs"].view(np.uint32), ref["probs"].cpu().numpy().view(np.uint32))
        np.testing.assert_array_equal(rec["labels"], ref["labels"].cpu().numpy())
    m._release()


def test_example_scan_prints_three_rows(capsys):
    spec = importlib.util.spec_from_file_location("classify_capture", os.path.join(ROOT, "examples", "classify_capture.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    model = VTCNN2.synthetic("deployed3")
    found = ex.scan(model, ex.synthetic_band("ci16"), "ci16", rate=2.4e6)
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(found) == 3 and lines[0].startswith("3 emitters (Hz)") and len(lines) == 2 + 3
    for line, fc in zip(lines[2:], S.BAND_CENTRES):
        assert abs(float(line.split()[0]) - fc * 2.4e6) < 0.001 * 2.4e6
    model._release()
