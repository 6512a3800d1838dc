"""mdc_iq_balance_blocks / mdc_iq_balance_stats / mdc_iq_balance and frontend.design_balance / image_rejection_db without a GPU:

  1. the reference (tests/iq_balance_ref.py) against itself and frontend's design against the reference: a balanced capture
     gives the identity and zero DC; a planted (gain, phase, dc) gives an image_rejection_db within 0.05 dB of the closed form
     20 log10 |K1 / K2| -- (1 dB, 5 degrees) and (0.2 dB, 1 degree) on 2^18 pairs: the estimate's own error there is 0.001 ..
     0.005 dB --; the correction brings a tone's image down to the noise floor, within 1 dB, in all three formats;
  2. design_balance: the row-sum rescale on a 6 dB imbalance, round-half-up DC at +-0.5, one summed row == the block rows;
  3. the three entries' argument validation (-22 and mdc_last_error's text, before any device call);
  4. the swap and conjugate matrices through the reference;
  5. the ghost scene of test_iq_balance_gpu.py through the CPU references: the strong emitter's image is an emitter of the
     scan's search before the correction and none after it, with margins printed here and stated in the test."""
import ctypes
import math

import numpy as np
import pytest

import iq_balance_ref as R
import iq_spectrum_ref as S
from modulationdetectioncnn_amd import _cabi, frontend

FORMATS = ["cu8", "ci8", "ci16"]
PAIRS = 1 << 18


def _scene(seed=3, pairs=PAIRS, amp=0.25, noise_rms=2.0e-4):
    """a tone at +0.1837, a weaker one at -0.31 and complex noise, in float, |.| < 0.5 per rail"""
    rng = np.random.default_rng(seed)
    n = np.arange(pairs)
    z = amp * np.exp(2j * np.pi * (0.1837 * n + 0.3)) + 0.1 * amp * np.exp(2j * np.pi * (-0.31 * n + 0.1))
    return z + noise_rms / math.sqrt(2.0) * (rng.standard_normal(pairs) + 1j * rng.standard_normal(pairs))


def _welch(iq, fmt, nfft=1024):
    """mean Hann periodogram over disjoint segments of the widened capture: (nfft,) float64"""
    x, y = R.widen(iq, fmt)
    z = (x + 1j * y).astype(np.complex128)
    z = z[:z.size // nfft * nfft].reshape(-1, nfft) * np.hanning(nfft)[None, :]
    return (np.abs(np.fft.fft(z, axis=1)) ** 2).mean(axis=0)


def test_names_and_limits_are_bound():
    assert {"mdc_iq_balance", "mdc_iq_balance_stats", "mdc_iq_balance_blocks"} <= set(_cabi.EXPORTS)
    assert _cabi.BALANCE_MIN_BLOCK == R.MIN_BLOCK == 64 and _cabi.BALANCE_MAX_BLOCK == R.MAX_BLOCK == 1 << 20
    assert _cabi.IQ_BALANCE_COEFFS.itemsize == 24 and _cabi.ABI_VERSION == 5
    assert tuple(frontend.BALANCE_IDENTITY)[:6] == R.IDENTITY and tuple(frontend.BALANCE_SWAP)[:6] == R.SWAP
    assert tuple(frontend.BALANCE_CONJUGATE)[:6] == R.CONJUGATE


def test_balanced_capture_gives_identity_and_zero_dc():
    iq = R.quantise(_scene(), "ci16")
    sums = R.stats(iq, "ci16", 65536)
    assert sums.shape == (4, 5)
    assert R.design(sums, PAIRS) == R.IDENTITY + (1.0,)
    assert frontend.design_balance(sums, PAIRS) == frontend.BALANCE_IDENTITY
    assert R.image_rejection_db(sums, PAIRS) > 80.0 and frontend.image_rejection_db(sums, PAIRS) == pytest.approx(R.image_rejection_db(sums, PAIRS), abs=1e-6)
    assert np.array_equal(R.correct(iq, "ci16", R.IDENTITY).reshape(-1), iq)


@pytest.mark.parametrize("gain_db,phase_deg", [(1.0, 5.0), (0.2, 1.0)])
def test_planted_imbalance_is_measured_to_the_closed_form(gain_db, phase_deg):
    iq = R.quantise(R.impair(_scene(), gain_db, phase_deg, 0.01 - 0.02j), "ci16")
    sums = R.stats(iq, "ci16", 4099)
    want = R.closed_form_irr_db(gain_db, phase_deg)
    got_ref, got = R.image_rejection_db(sums, PAIRS), frontend.image_rejection_db(sums, PAIRS)
    print(f"{gain_db} dB / {phase_deg} deg: closed form {want:.4f} dB, reference {got_ref:.4f} dB, frontend {got:.4f} dB")
    assert abs(got_ref - want) <= 0.05 and abs(got - want) <= 0.05
    if (gain_db, phase_deg) == (1.0, 5.0):
        assert want == pytest.approx(22.83, abs=0.005)
    c = frontend.design_balance(sums, PAIRS)
    assert tuple(c) == R.design(sums, PAIRS)
    assert (c.dc_i, c.dc_q) == (328, -655)      # 0.01 and -0.02 of 32768, round half up
    # the corrected capture's own statistics: balanced to the quantiser's grain
    fixed = R.correct(iq, "ci16", c).reshape(-1)
    after = R.stats(fixed, "ci16", 65536)
    assert R.image_rejection_db(after, PAIRS) > want + 30.0
    assert tuple(frontend.design_balance(after, PAIRS))[:2] == (0, 0)


@pytest.mark.parametrize("fmt", FORMATS)
def test_correction_brings_the_image_down_to_the_floor(fmt):
    """The tone at +0.1837 leaves an image at -0.1837, 22.8 dB below it; corrected, what stands in the image's bins is the noise
    floor: the mean of the five bins around the mirror against the mean of a band that holds nothing, within 1 dB (disjoint
    Hann segments, 256 of them: a bin's mean scatters by 0.27 dB, five bins' by less)."""
    # noise of 2.5e-3 rms puts the floor some 60 dB below the tone in every format (an 8-bit quantiser adds 1.1e-3 per rail).  Far
    # lower floors meet the correction's own grain: Q14 coefficients (half a step is 3e-5: an image near -90 dB) and the
    # estimate's noise, so a floor 85 dB down is no longer reached to within 1 dB
    iq = R.quantise(R.impair(_scene(noise_rms=2.5e-3), 1.0, 5.0, 0.01 - 0.02j), fmt, full_scale=0.5)
    p = _welch(iq, fmt)
    k, mirror = round(0.1837 * 1024), 1024 - round(0.1837 * 1024)
    before = 10 * math.log10(p[k - 2:k + 3].sum() / p[mirror - 2:mirror + 3].sum())
    assert abs(before - 22.83) < 0.3
    sums = R.stats(iq, fmt, 65536)
    fixed = R.correct(iq, fmt, R.design(sums, PAIRS)).reshape(-1)
    q = _welch(fixed, "ci16")
    quiet = np.r_[380:480]      # +0.37 .. +0.47: no tone, no image, far from every leakage skirt
    tone = q[k - 2:k + 3].sum()
    to_image = 10 * math.log10(tone / q[mirror - 2:mirror + 3].sum())
    to_floor = 10 * math.log10(tone / (5 * q[quiet].mean()))
    print(f"{fmt}: image {before:.2f} dB below the tone before, {to_image:.2f} dB after; floor {to_floor:.2f} dB below the tone")
    assert to_floor > 50.0 and abs(to_image - to_floor) <= 1.0


def test_design_rescales_rows_beyond_q14_range():
    """A rail's gain in M is sqrt((1 + g^2) / 2) for the weak rail of a gain ratio g (the total power is kept): Q14 holds it up
    to 2, that is g < sqrt(7), 8.45 dB.  6 dB (1.58) therefore still fits as designed; 10 dB (2.35) takes the rescale, and the
    result says so."""
    iq = R.quantise(R.impair(_scene(amp=0.1), 6.0, 3.0), "ci16")
    sums = R.stats(iq, "ci16", 65536)
    c = frontend.design_balance(sums, PAIRS)
    assert tuple(c) == R.design(sums, PAIRS) and c.scale == 1.0
    assert 1.5 * 16384 < c.m00 < 1.65 * 16384 and abs(c.m00) + abs(c.m01) <= 32767
    assert R.image_rejection_db(R.stats(R.correct(iq, "ci16", c).reshape(-1), "ci16", 65536), PAIRS) > 60.0
    iq = R.quantise(R.impair(_scene(amp=0.05), 10.0, 3.0), "ci16")
    sums = R.stats(iq, "ci16", 65536)
    c = frontend.design_balance(sums, PAIRS)
    assert tuple(c) == R.design(sums, PAIRS)
    assert 0.8 < c.scale < 1.0
    rows = (abs(c.m00) + abs(c.m01), abs(c.m10) + abs(c.m11))
    assert max(rows) <= 32767 and max(rows) >= 32760      # scaled no further than needed
    fixed = R.correct(iq, "ci16", c).reshape(-1)
    assert R.image_rejection_db(R.stats(fixed, "ci16", 65536), PAIRS) > 60.0      # a common scale does not unbalance


def test_dc_rounds_half_up():
    for n, Sx, Sy, want in ((2, 1, -1, (1, 0)), (2, 3, -3, (2, -1)), (4, 2, -2, (1, 0)), (4, 1, -1, (0, 0)), (4, -3, 3, (-1, 1))):
        row = np.array([Sx, Sy, 10 ** 6, 10 ** 6, 0], np.int64)
        c = frontend.design_balance(row, pairs=n)
        assert (c.dc_i, c.dc_q) == want == R.design(row, n)[:2], (n, Sx, Sy)


def test_one_summed_row_equals_the_block_rows():
    iq = R.quantise(R.impair(_scene(pairs=50_001), 0.7, -3.0, 0.02 + 0.01j), "ci16")
    blocks = R.stats(iq, "ci16", 1027)
    assert blocks.shape == (49, 5)
    assert np.array_equal(blocks.sum(axis=0), R.stats(iq, "ci16", 1 << 20)[0])
    assert frontend.design_balance(blocks, 50_001) == frontend.design_balance(blocks.sum(axis=0), 50_001)
    assert frontend.image_rejection_db(blocks, 50_001) == frontend.image_rejection_db(blocks.sum(axis=0), 50_001)
    with pytest.raises(ValueError, match="pairs"):
        frontend.design_balance(blocks)
    assert frontend.design_balance(np.zeros((0, 5), np.int64), 0) == frontend.BALANCE_IDENTITY
    assert frontend.image_rejection_db(np.zeros((0, 5), np.int64), 0) == math.inf


def test_swap_and_conjugate_matrices():
    rng = np.random.default_rng(5)
    for fmt in FORMATS:
        iq = rng.integers(R.SAMPLE_MIN[fmt], R.SAMPLE_MAX[fmt] + 1, size=2000).astype(R.DTYPE[fmt])
        x, y = R.widen(iq, fmt)
        assert np.array_equal(R.correct(iq, fmt, R.IDENTITY), np.stack([x, y], axis=1))
        assert np.array_equal(R.correct(iq, fmt, R.SWAP), np.stack([y, x], axis=1))
        assert np.array_equal(R.correct(iq, fmt, R.CONJUGATE), np.stack([x, np.minimum(-y, 32767)], axis=1))
    # the swap inverts the spectrum: a tone at +f comes out at -f
    n = np.arange(4096)
    tone = R.quantise(0.5 * np.exp(2j * np.pi * 0.125 * n), "ci16")
    z = R.correct(tone, "ci16", R.SWAP).astype(np.float64)
    assert np.argmax(np.abs(np.fft.fft(z[:, 0] + 1j * z[:, 1]))) == 4096 - 512


def test_blocks_entry():
    L = _cabi.lib()
    for B in (64, 65, 1027, 1 << 20):
        for pairs in (0, 1, B - 1, B, B + 1, 3 * B + 7):
            assert L.mdc_iq_balance_blocks(pairs, B) == R.blocks(pairs, B) == frontend.balance_blocks(pairs, B)
    for B in (0, 1, 63, (1 << 20) + 1, -64):
        assert L.mdc_iq_balance_blocks(100, B) == -22 and b"block_pairs must be in 64..1048576" in L.mdc_last_error()
    assert L.mdc_iq_balance_blocks(-1, 64) == -22 and b"negative pair count" in L.mdc_last_error()
    with pytest.raises(_cabi.MdcError):
        frontend.balance_blocks(10, 63)


def test_stats_entry_validates_its_arguments_without_gpu():
    L = _cabi.lib()
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.addressof(buf)

    def call(iq=p, fmt=2, pairs=100, B=64, sums=p, nblocks=2):
        return L.mdc_iq_balance_stats(iq, fmt, pairs, B, sums, nblocks, None)
    assert call(fmt=3) == -22 and b"unknown sample format" in L.mdc_last_error()
    assert call(fmt=-1) == -22 and b"unknown sample format" in L.mdc_last_error()
    assert call(pairs=-1) == -22 and b"negative pair count" in L.mdc_last_error()
    assert call(B=63) == -22 and b"block_pairs" in L.mdc_last_error()
    assert call(B=(1 << 20) + 1) == -22 and b"block_pairs" in L.mdc_last_error()
    assert call(nblocks=1) == -22 and b"nblocks is 1, mdc_iq_balance_blocks gives 2" in L.mdc_last_error()
    assert call(nblocks=3) == -22 and b"nblocks" in L.mdc_last_error()
    assert call(iq=p + 2) == -22 and b"whole (I,Q) pair" in L.mdc_last_error()
    assert call(iq=p + 1, fmt=0) == -22 and b"whole (I,Q) pair" in L.mdc_last_error()
    assert call(sums=p + 4) == -22 and b"8-byte aligned" in L.mdc_last_error()
    assert call(iq=None) == -22 and b"null buffer" in L.mdc_last_error()
    assert call(sums=None) == -22 and b"null buffer" in L.mdc_last_error()
    assert call(iq=None, sums=None, pairs=0, nblocks=0) == 0      # nothing to do, nothing launched
    assert call(pairs=0, nblocks=1) == -22


def test_balance_entry_validates_its_arguments_without_gpu():
    L = _cabi.lib()
    buf = (ctypes.c_int32 * 256)()
    p = ctypes.addressof(buf)
    out = p + 512

    def call(iq=p, fmt=2, pairs=100, c=R.IDENTITY, out=out):
        rec = None
        if c is not None:
            rec = np.zeros((), _cabi.IQ_BALANCE_COEFFS)
            for name, v in zip(_cabi.IQ_BALANCE_COEFFS.names, c):
                rec[name] = v
        return L.mdc_iq_balance(iq, fmt, pairs, rec.ctypes.data if rec is not None else None, out, None)
    assert call(fmt=7) == -22 and b"unknown sample format" in L.mdc_last_error()
    assert call(pairs=-5) == -22 and b"negative pair count" in L.mdc_last_error()
    assert call(c=None) == -22 and b"null coefficients" in L.mdc_last_error()
    for bad in ((32769, 0), (0, -32769)):
        assert call(c=bad + R.IDENTITY[2:]) == -22 and b"-32768..32768" in L.mdc_last_error()
    for row in ((32767, 1), (-16384, 16384), (0, -32768)):
        assert call(c=(0, 0) + row + (16384, 0)) == -22 and b"at most 32767" in L.mdc_last_error()
        assert call(c=(0, 0, 16384, 0) + row) == -22 and b"at most 32767" in L.mdc_last_error()
    assert call(iq=p + 2) == -22 and b"whole (I,Q) pair" in L.mdc_last_error()
    assert call(out=out + 2) == -22 and b"4-byte aligned" in L.mdc_last_error()
    assert call(iq=None) == -22 and b"null buffer" in L.mdc_last_error()
    assert call(out=None) == -22 and b"null buffer" in L.mdc_last_error()
    assert call(out=p + 396) == -22 and b"overlap" in L.mdc_last_error()      # the input's last pair
    assert call(fmt=0, out=p + 196) == -22 and b"overlap" in L.mdc_last_error()
    assert call(iq=None, out=None, pairs=0) == 0
    assert call(iq=None, out=None, pairs=0, c=(32768, -32768, 32767, 0, 16384, -16383)) == 0      # the extremes are legal
    with pytest.raises(ValueError):
        frontend._balance_record((0, 0, 1))


def test_ghost_scene_holds_through_the_cpu_references():
    """What test_iq_balance_gpu.py asks of scan_iq, through iq_balance_ref + iq_spectrum_ref + frontend.find_emitters: margins
    seen here -- the image 18.4 dB above the floor before the correction (threshold: 6 dB), 0.1 dB after it."""
    iq = R.ghost_scene()
    pairs = iq.size // 2
    w = frontend.design_window(1024)

    def emitters(x):
        psd = S.band_psd(x, 1024, w, frontend.window_scale(w))
        return frontend.find_emitters(psd, threshold_db=6.0, window=w), psd
    sps, fc, _ = R.GHOST_STRONG
    half = 1.35 / sps / 2
    raw, psd0 = emitters(iq)
    ghosts = [e for e in raw if abs(e.centre + fc) <= half]
    assert len(raw) == 3 and len(ghosts) == 1 and ghosts[0].snr_db > 12.0
    sums = R.stats(iq, "ci16", 65536)
    assert abs(R.image_rejection_db(sums, pairs) - 22.83) <= 0.5
    fixed, psd1 = emitters(R.correct(iq, "ci16", R.design(sums, pairs)).reshape(-1))
    assert len(fixed) == 2 and not [e for e in fixed if abs(e.centre + fc) <= 2 * half]
    k = round(-fc * 1024) % 1024
    print(f"image bin over the median: {10 * math.log10(psd0[k] / np.median(psd0)):.2f} dB before, {10 * math.log10(psd1[k] / np.median(psd1)):.2f} dB after")
    assert 10 * math.log10(psd1[k] / np.median(psd1)) < 3.0
    kept = [e for e in raw if abs(e.centre + fc) > half]
    for a, b in zip(kept, fixed):
        assert abs(a.centre - b.centre) <= 1.0 / 1024
