"""mdc_iq_channelizer / frontend.channelize / VTCNN2.predict_channels on the MI355X, against tests/iq_channelizer_ref.py (float64
numpy, written from include/mdc.h):

  1. parity: M in 8..1024 (every pass structure of the mixed-radix transform, the sizes below the spectrogram's) x the three
     formats x D in {M, M/2, 3} x three tap sets (design_channelizer; random asymmetric taps of T = 3 M + 5, ragged residues, scaled
     to the per-residue limit; T = M - 3, where some residues are empty) x first_index in {0, 5}, on a capture giving n_out = 37,
     on pairs == T (one column) and pairs == T - 1 (none); the base pointer one pair into a larger allocation; the output
     pre-filled with a sentinel and a guard row after the last channel untouched (the rows are contiguous, M rows of n_out pairs:
     the pair after row k IS row k + 1's first, which the comparison itself covers; only the last row has room behind it); inputs uniform
     over the full range with planted runs of all-minimum, all-maximum and alternating pairs, two tones, and a full-scale run whose
     signs follow sign(h), so that channel 0 must clamp.  The tolerance is the header's, every term from the reference:
         |out - clamp(Y)| <= 0.5 + eps S_j,  u = 2^-24, eps = 8u (log2 M + 1)
     (Y, S_j in output LSB; a float32 restatement on the CPU stayed below 0.002 LSB of the unrounded Y, the bound allows 0.17 at
     M = 1024 on a full-scale tone);
  2. the same call twice gives the same bits; a call from pair 7 D on with first_index + 7 D is columns 7.. of the whole call;
  3. every channel row within 2 LSB of the exact down-converter on the device (frontend.ddc with the matching step and phase0);
  4. past the grid cap: first, last, the columns around each multiple of cap x tile and 200 random columns against the reference,
     the whole output against a two-piece run split off the cap's grid;
  5. frontend.channelize with its cached taps replays bit-identically from a captured graph after the input is overwritten;
  6. VTCNN2.predict_channels against channelising and classifying by hand, a synthetic band with QPSK on two channels, and the
     example's --channels path."""
import functools
import importlib.util
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import iq_channelizer_ref as R                                                           # noqa: E402
import iq_spectrum_ref as S                                                              # noqa: E402
import signals                                                                           # noqa: E402
from conftest import GOLDEN, ROOT                                                        # noqa: E402
from modulationdetectioncnn_amd import VTCNN2, _cabi, frontend                           # noqa: E402

FORMATS = ["cu8", "ci8", "ci16"]
CHANNELS = [8, 16, 32, 64, 128, 256, 512, 1024]
SENTINEL = -21846                                                                        # 0xAAAA


def _capture(fmt, pairs, seed, plant=None):
    """One pair of padding + `pairs` pairs + one pair of padding.  Uniform over the whole range; from the middle on two tones,
    0.6 and 0.006 of full scale; runs of 300 pairs of all minimum, all maximum and alternating minimum / maximum pairs at pairs 0,
    700, 1500 and 200 before the end (cut off where the capture is shorter).  plant = (at, taps): from pair `at` on I is the
    maximum where the tap is >= 0 and the minimum where it is negative, Q the opposite -- the column starting there is
    sum |h| times full scale on channel 0, whose phase factor is 1 for every index."""
    lo, hi, dt = R.SAMPLE_MIN[fmt], R.SAMPLE_MAX[fmt], R.DTYPE[fmt]
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
    if plant is not None:
        at, taps = plant
        if at + taps.size <= pairs:
            seg = body[2 * at: 2 * (at + taps.size)]
            seg[0::2] = np.where(taps >= 0, hi, lo)
            seg[1::2] = np.where(taps >= 0, lo, hi)
    return buf


def _random_taps(M, T, seed):
    """asymmetric int16 taps (a reversed or shifted index shows), scaled so that the largest residue's sum |h| is just inside 65535"""
    h = np.random.default_rng(seed).integers(-32768, 32768, size=T).astype(np.float64)
    worst = max(np.abs(h[r::M]).sum() for r in range(min(M, T)))
    q = np.trunc(h * min(1.0, 65535.0 / worst)).astype(np.int16)
    R.check_taps(q, M)
    return q


def _tap_sets(M):
    h, shift = frontend.design_channelizer(M)
    return [(h, shift), (_random_taps(M, 3 * M + 5, seed=M), int(np.log2(M)) - 1), (_random_taps(M, M - 3, seed=M + 1), 0)]


def _channelize(dev, fmt, pairs, first, M, D, hdev, T, shift):
    """mdc_iq_channelizer straight through the binding; dev: the device tensor whose data_ptr is pair 0.  Returns the (M, n_out, 2)
    device tensor after checking the guard row behind the last channel's."""
    L = _cabi.lib()
    n_out = L.mdc_iq_channelizer_out_count(pairs, M, T, D)
    assert n_out == R.out_count(pairs, T, D)
    out = torch.full((M + 1, n_out, 2), SENTINEL, dtype=torch.int16, device="cuda")
    _cabi.check(L.mdc_iq_channelizer(dev.data_ptr(), S.FMT[fmt], pairs, first, M, D, hdev.data_ptr(), T, shift, out.data_ptr(), n_out,
                                     torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert bool((out[M] == SENTINEL).all())
    return out[:M]


def _worst_ratio(got, iq, fmt, first, M, D, taps, shift, columns=None):
    """largest |got - clamp(Y)| / bound over the columns (all, or the listed ones), every term of the bound from the float64 reference"""
    Y, Sj = R.channelize(iq, fmt, first, M, D, taps, shift, columns)
    assert got.shape == (M, Y.shape[1], 2)
    if Y.size == 0:
        return 0.0, Y
    re, im = R.clamped(Y)
    err = np.maximum(np.abs(got[:, :, 0].astype(np.float64) - re), np.abs(got[:, :, 1].astype(np.float64) - im))
    return float((err / R.bound(Sj, M)[None, :]).max()), Y


# ---------------------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("M", CHANNELS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_channelizer_is_the_reference(fmt, M):
    worst, clamped_high, clamped_low = 0.0, 0, 0
    for taps, shift in _tap_sets(M):
        T = taps.size
        hdev = torch.from_numpy(taps).cuda()
        for D in (M, M // 2, 3):
            for first in (0, 5):
                for pairs in ((T + 36 * D, T, T - 1) if first == 5 else (T + 36 * D + D - 1,)):
                    jp = 20                                                  # the planted column
                    buf = _capture(fmt, pairs, seed=M + D + pairs + first, plant=(jp * D, taps))
                    dev = torch.from_numpy(buf).cuda()[2:]                   # one pair into the allocation
                    assert dev.data_ptr() % 256 == _cabi.IQ_PAIR_BYTES[S.FMT[fmt]]
                    got = _channelize(dev, fmt, pairs, first, M, D, hdev, T, shift).cpu().numpy()
                    assert got.shape == (M, 37 if pairs > T else 1 if pairs == T else 0, 2)
                    ratio, Y = _worst_ratio(got, buf[2:2 + 2 * pairs], fmt, first, M, D, taps, shift)
                    worst = max(worst, ratio)
                    assert ratio <= 1.0, (fmt, M, D, T, first, pairs, ratio)
                    if pairs > T:
                        # the planted column: channel 0 is sum |h| times full scale whatever first_index is, and clamps both ways
                        assert Y[0, jp].real > 32767.5 and Y[0, jp].imag < -32768.5, (fmt, M, D, T, first, Y[0, jp])
                        assert tuple(got[0, jp]) == (32767, -32768)
                        clamped_high += int((got == 32767).sum())
                        clamped_low += int((got == -32768).sum())
    assert clamped_high > 0 and clamped_low > 0
    print(f"{fmt} M {M}: largest error / bound {worst:.4f}")


# ---------------------------------------------------------------------------------------------------------------- 2. determinism, pieces
@pytest.mark.parametrize("M", [16, 1024])
@pytest.mark.parametrize("fmt", FORMATS)
def test_determinism_and_piece_identity(fmt, M):
    D, first = M // 2 + 1, 3
    taps, shift = _random_taps(M, 5 * M + 7, seed=7), int(np.log2(M)) - 1
    T = taps.size
    pairs = T + 40 * D + 2
    buf = _capture(fmt, pairs, seed=M)
    dev = torch.from_numpy(buf).cuda()[2:]
    hdev = torch.from_numpy(taps).cuda()
    whole = _channelize(dev, fmt, pairs, first, M, D, hdev, T, shift)
    assert whole.shape == (M, 41, 2)
    assert torch.equal(whole, _channelize(dev, fmt, pairs, first, M, D, hdev, T, shift))
    ratio, _ = _worst_ratio(whole.cpu().numpy(), buf[2:2 + 2 * pairs], fmt, first, M, D, taps, shift)
    assert ratio <= 1.0
    a = 7 * D
    pb = _cabi.IQ_PAIR_BYTES[S.FMT[fmt]] // buf.itemsize                     # elements per pair
    piece = _channelize(dev[pb * a:], fmt, pairs - a, first + a, M, D, hdev, T, shift)
    assert piece.shape == (M, 34, 2) and torch.equal(piece, whole[:, 7:])
    for j in (0, 11, 40):                                                     # a column does not depend on what else the call computes
        one = _channelize(dev[pb * j * D:], fmt, T, first + j * D, M, D, hdev, T, shift)
        assert one.shape == (M, 1, 2) and torch.equal(one[:, 0], whole[:, j]), (fmt, M, j)


# ---------------------------------------------------------------------------------------------------------------- 3. the exact down-converter
def test_every_channel_is_the_down_converter_within_two_lsb():
    M, D, T, first = 64, 32, 512, 5
    taps = frontend.design_lowpass(D, ntaps=T, cutoff=0.5 / M)                # Q15, unit sum: tap_shift 0
    pairs = T + 127 * D
    g = torch.Generator(device="cuda").manual_seed(3)
    dev = torch.randint(-32768, 32768, (2 * pairs,), dtype=torch.int16, device="cuda", generator=g)
    bank = frontend.channelize(dev, "ci16", M, decimate=D, taps=taps, tap_shift=0, first_index=first)
    assert bank.shape == (M, 128, 2)
    worst = 0
    for k in range(M):
        shift = -k / M if 2 * k <= M else (M - k) / M                         # -k/M cycles per sample, folded into [-0.5, 0.5]
        step = frontend.phase_step(shift)
        assert step == (-k * (1 << 32) // M) % (1 << 32)
        down = frontend.ddc(dev, "ci16", shift=shift, decimate=D, taps=taps, phase0=(first * step) % (1 << 32))
        worst = max(worst, int((bank[k].to(torch.int32) - down.to(torch.int32)).abs().max()))
    print(f"largest |channelizer - ddc| over {M} channels: {worst} LSB")
    assert worst <= 2


# ---------------------------------------------------------------------------------------------------------------- 4. past the grid cap
def test_stride_loop_past_the_grid_cap():
    M, T, D, fmt, first = 8, 8, 8, "cu8", 3
    cap, tile = _cabi.CHANNELIZER_GRID_CAP, _cabi.channelizer_tile_steps(M)
    n_out = 2 * cap * tile + 5 * tile + 7
    pairs = T + (n_out - 1) * D
    g = torch.Generator(device="cuda").manual_seed(4)
    dev = torch.randint(0, 256, (2 * pairs,), dtype=torch.uint8, device="cuda", generator=g)
    iq = dev.cpu().numpy()
    taps, shift = _random_taps(M, T, seed=9), 0
    hdev = torch.from_numpy(taps).cuda()
    whole = _channelize(dev, fmt, pairs, first, M, D, hdev, T, shift)
    assert whole.shape == (M, n_out, 2)
    rng = np.random.default_rng(8)
    edges = [m * cap * tile + d for m in (1, 2) for d in (-tile, -1, 0, 1, tile - 1, tile)]
    picks = np.unique(np.concatenate([[0, n_out - 1], edges, rng.integers(0, n_out, size=200)]))
    ratio, _ = _worst_ratio(whole[:, torch.from_numpy(picks).cuda()].cpu().numpy(), iq, fmt, first, M, D, taps, shift, columns=picks)
    print(f"largest error / bound {ratio:.4f}")
    assert ratio <= 1.0
    cols = (cap // 2 + 123) * tile + 17                                       # columns of the first piece: the second piece's tiles start off the cap's
    one = _channelize(dev, fmt, T + (cols - 1) * D, first, M, D, hdev, T, shift)
    two = _channelize(dev[2 * cols * D:], fmt, pairs - cols * D, first + cols * D, M, D, hdev, T, shift)
    assert one.shape[1] == cols and torch.equal(torch.cat([one, two], dim=1), whole)


# ---------------------------------------------------------------------------------------------------------------- 5. graph capture
def test_channelize_is_capturable():
    M, fmt = 64, "ci16"
    pairs = 8 * M + 300 * (M // 2)
    dev = torch.from_numpy(_capture(fmt, pairs, seed=1)[2:-2].copy()).cuda()
    frontend.channelize(dev, fmt, M)                               # warm: the cached taps, code objects
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        c1 = frontend.channelize(dev, fmt, M)
    assert c1.shape == (M, 301, 2)
    for seed in (2, 3):
        dev.copy_(torch.from_numpy(_capture(fmt, pairs, seed=seed)[2:-2].copy()).cuda())      # same buffer, new capture
        c1.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        ce = frontend.channelize(dev, fmt, M)
        torch.cuda.synchronize()
        assert torch.equal(c1, ce) and not bool((ce == SENTINEL).all()), seed


# ---------------------------------------------------------------------------------------------------------------- 6. end to end
BAND_M, BAND_ON, BAND_AMPLITUDE, BAND_NOISE_RMS = 16, (3, 11), 0.05, 0.002


@functools.lru_cache(maxsize=None)
def _raster_band():
    """ci16: QPSK (tests/signals.py's constellation) through tests/iq_spectrum_ref.py's root-raised-cosine pulse at 64 samples per
    symbol -- 8 per symbol after D = M / 2 = 8 --, rms 0.05 of full scale, on channels 3 and 11 of a 16-channel raster, over complex
    noise of rms 0.002.  Shared: nobody writes to it."""
    rng = np.random.default_rng(16)
    M, sps = BAND_M, 8 * (BAND_M // 2)
    pairs = 8 * M + (12 * 128 - 1) * (M // 2) + 40                            # 12 whole frames per channel and a little more
    n, z = np.arange(pairs), np.zeros(pairs, complex)
    pts = signals._constellation("QPSK")
    for k in BAND_ON:
        nsym = pairs // sps + 2
        up = np.zeros(nsym * sps, complex)
        up[::sps] = pts[rng.integers(0, 4, nsym)]
        base = np.convolve(up, S.rrc_pulse(sps), mode="same")[:pairs]
        z += BAND_AMPLITUDE / np.sqrt(np.mean(np.abs(base) ** 2)) * base * np.exp(2j * np.pi * k / M * n)
    z += BAND_NOISE_RMS / np.sqrt(2.0) * (rng.standard_normal(pairs) + 1j * rng.standard_normal(pairs))
    v = np.stack([z.real, z.imag], axis=1) * 32768.0
    iq = np.clip(np.rint(v), -32768, 32767).astype(np.dtype("<i2")).reshape(-1)
    return iq


@functools.lru_cache(maxsize=None)
def _model():
    return VTCNN2.from_npz(os.path.join(GOLDEN, "weights", "3convmodrecnets_CNN2_0.5.npz"))


@pytest.mark.parametrize("hop", [128, 64])
def test_predict_channels_is_channelize_and_predict_by_hand(hop):
    iq, m, M, squelch = _raster_band(), _model(), BAND_M, -45.0
    dev = torch.from_numpy(iq.copy()).cuda()
    probs, labels, dbfs, label = m.predict_channels(dev, "ci16", M, hop=hop, squelch_dbfs=squelch)
    down = frontend.channelize(dev, "ci16", M, whole_frames=True)
    assert down.shape == (M, 12 * 128, 2)
    W = 12 if hop == 128 else (12 * 128 - 128) // hop + 1
    assert probs.shape == (M, W, m.topology.classes) and labels.shape == dbfs.shape == (M, W) and label.shape == (M,)
    for k in range(M):
        p, l, d = m.predict_iq(down[k].reshape(-1), "ci16", hop=hop, normalize="rms", level=7.8e-3, squelch_dbfs=squelch, return_power=True)
        assert torch.equal(probs[k], p) and torch.equal(labels[k], l) and torch.equal(dbfs[k], d), k
        open_ = l[l >= 0]
        assert int(label[k]) == (int(torch.bincount(open_).argmax()) if open_.numel() else -1)
    by_numpy = m.predict_channels(iq, "ci16", M, hop=hop, squelch_dbfs=squelch)           # numpy in, numpy out
    for got, ref in zip(by_numpy, (probs, labels, dbfs, label)):
        assert isinstance(got, np.ndarray)
        np.testing.assert_array_equal(got.view(np.uint8), ref.cpu().numpy().view(np.uint8))


def test_occupied_channels_stand_out_and_empty_ones_are_squelched():
    iq, m, M = _raster_band(), _model(), BAND_M
    _, labels, dbfs, label = m.predict_channels(iq, "ci16", M, squelch_dbfs=-45.0)
    median = np.median(dbfs, axis=1)
    on = np.zeros(M, bool)
    on[list(BAND_ON)] = True
    print("median window dBFS per channel:", np.round(median, 1), "labels:", label)
    assert median[on].min() >= median[~on].max() + 30.0
    assert median[on].min() > -45.0 > median[~on].max()                       # the squelch lies between the two levels
    assert np.all(label[~on] == -1) and np.all(labels[~on] == -1)
    assert np.all(label[on] >= 0) and np.all(labels[on] >= 0)
    assert abs(median[on] - 20.0 * np.log10(BAND_AMPLITUDE)).max() < 1.0      # the channel's gain is 1: rms 0.05 reads -26 dBFS


def test_example_channels_prints_one_line_per_channel(capsys):
    spec = importlib.util.spec_from_file_location("classify_capture", os.path.join(ROOT, "examples", "classify_capture.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    model = VTCNN2.synthetic("deployed3")
    M, rate = 16, 2.4e6
    labels, dbfs, label = ex.channels(model, ex.synthetic_raster("ci16", M), "ci16", M, rate=rate, squelch=-45.0)
    lines = capsys.readouterr().out.strip().splitlines()
    assert lines[0].startswith(f"{M} channels (Hz)") and len(lines) == 2 + M and label.shape == (M,)
    for line, fc in zip(lines[2:], frontend.channel_freqs(M)):
        assert abs(float(line.split()[0]) - fc * rate) < 1.0
    assert sorted(np.flatnonzero(label >= 0)) == [3, 11]
    model._release()
