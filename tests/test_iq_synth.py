"""Frame synthesis on the host (no GPU): mdc_iq_synth_plan's validation through the C ABI, the label raster, and statistical
checks of the numpy restatement (tests/iq_synth_ref.py) against the design's exact expectations -- margins derived, not tuned:
every comparison is 5 standard errors of the sample's own per-frame means."""
import ctypes

import numpy as np
import pytest

import iq_synth_ref as ref
from modulationdetectioncnn_amd import _cabi, frontend

FRAMES = 4096          # per statistical check
LINEAR_MODS = ("BPSK", "QPSK", "8PSK", "PAM4", "QAM16", "QAM64")


def _err():
    return _cabi.lib().mdc_last_error().decode()


def small_tables(**over):
    """a valid one-class recipe (an alphabet of two points, sps 2, span 2) as mdc_iq_synth_plan's arguments; `over` replaces fields
    of the class record"""
    cl = np.zeros(1, _cabi.IQ_SYNTH_CLASS)
    cl[0]["source"], cl[0]["points"], cl[0]["sps"], cl[0]["span"], cl[0]["mode"] = _cabi.SYNTH_ALPHABET, 2, 2, 2, _cabi.SYNTH_LINEAR
    for k, v in over.items():
        cl[0][k] = v
    pts = np.array([[1000, 0], [-1000, 0]], np.int16)
    taps = np.array([[8000, 0], [4000, -100], [2000, 50], [1000, 0]], np.int16)
    return dict(classes=cl, points=pts, taps=taps, gain_sig=np.full((1, 3), 1 << 16, np.int32), gain_noise=np.full(3, 100, np.int32),
                max_step=1 << 20, q=16)


def plan_rc(t, plan_bytes=None, ngain_sig=None, nsnrs=None):
    """(rc of mdc_iq_synth_plan, blob) with the tables of small_tables; the keyword arguments lie about a size"""
    L = _cabi.lib()
    cl, S = t["classes"], t["gain_noise"].size if nsnrs is None else nsnrs
    nb = L.mdc_iq_synth_plan_bytes(cl.size, S, cl.ctypes.data)
    blob = np.zeros(max(int(nb), 16) + 64, np.uint8)
    gs = np.ascontiguousarray(t["gain_sig"], np.int32)
    rc = L.mdc_iq_synth_plan(cl.ctypes.data, cl.size, t["points"].ctypes.data, t["points"].shape[0], t["taps"].ctypes.data, t["taps"].shape[0],
                             gs.ctypes.data, gs.size if ngain_sig is None else ngain_sig, t["gain_noise"].ctypes.data, S, t["max_step"], t["q"],
                             blob.ctypes.data, nb if plan_bytes is None else plan_bytes)
    return rc, blob[:max(int(nb), 0)]


# ------------------------------------------------------------------------------------------------------------ 1. plan validation
def test_a_valid_plan_is_accepted_and_sized():
    t = small_tables()
    rc, blob = plan_rc(t)
    assert rc == 0, _err()
    assert blob.size % 16 == 0 and blob.size > 0
    assert int(blob[24:32].view(np.int64)[0]) == blob.size          # the header's own `bytes`
    assert frontend.synth_plan(**t).tobytes() == blob.tobytes()     # the same inputs give the same bytes


@pytest.mark.parametrize("points", [0, 3, 6, 12, 128, -2])
def test_alphabet_size_must_be_a_power_of_two(points):
    L = _cabi.lib()
    t = small_tables(points=points)
    assert L.mdc_iq_synth_plan_bytes(1, 3, t["classes"].ctypes.data) == -22 and "class 0: points must be a power of two" in _err()
    assert plan_rc(t)[0] == -22 and "power of two" in _err()


@pytest.mark.parametrize("field,value,text", [("sps", 0, "sps must be in 1..16"), ("sps", 17, "sps must be in 1..16"),
                                              ("span", 0, "span must be in 1..16"), ("span", 17, "span must be in 1..16"),
                                              ("source", 2, "unknown source"), ("mode", 2, "unknown mode"), ("reserved", 1, "reserved must be 0"),
                                              ("first_tap", -1, "negative first_point or first_tap")])
def test_class_fields_out_of_range_are_refused(field, value, text):
    t = small_tables(**{field: value})
    assert plan_rc(t)[0] == -22 and text in _err() and "class 0" in _err()


def test_pulse_longer_than_128_taps_is_refused():
    t = small_tables(sps=16, span=9)
    assert plan_rc(t)[0] == -22 and "at most 128 taps" in _err()


def test_gaussian_source_takes_no_points():
    t = small_tables(source=_cabi.SYNTH_GAUSS, points=2)
    assert plan_rc(t)[0] == -22 and "0 for a Gaussian source" in _err()


def test_branch_sum_too_large_is_refused_at_the_exact_bound():
    # one tap per branch (span 1), alphabet peak 32767: y's bound is (|h| * 32767 + 2^14) >> 15
    t = small_tables(span=1)
    t["points"] = np.array([[32767, 0], [0, -32767]], np.int16)
    t["taps"] = np.array([[32767, 0], [0, 32767]], np.int16)
    assert plan_rc(t)[0] == 0, _err()                        # (32767 * 32767 + 16384) >> 15 = 32766
    t["classes"][0]["add_im"] = 1
    assert plan_rc(t)[0] == 0, _err()                        # 32766 + 1
    t["classes"][0]["add_im"] = -2
    assert plan_rc(t)[0] == -22 and "branch 0" in _err() and "more than 32767" in _err()
    t["classes"][0]["add_im"] = 0
    t["taps"] = np.array([[32767, 0], [20000, -20000]], np.int16)      # |re| + |im| of branch 1 is 40000
    assert plan_rc(t)[0] == -22 and "class 0: branch 1" in _err()
    # the Gaussian source's largest value is 262140: a branch of 4096 gives ((4096 * 262140 + 2^14) >> 15) = 32768
    g = small_tables(source=_cabi.SYNTH_GAUSS, points=0, span=1)
    g["taps"] = np.array([[4095, 0], [0, 4095]], np.int16)
    assert plan_rc(g)[0] == 0, _err()
    g["taps"] = np.array([[4095, 0], [4096, 0]], np.int16)
    assert plan_rc(g)[0] == -22 and "branch 1" in _err()


def test_phase_amplitude_plus_constant_is_bounded():
    t = small_tables(mode=_cabi.SYNTH_PHASE, amplitude=30000, add_re=2767)
    assert plan_rc(t)[0] == 0, _err()
    t = small_tables(mode=_cabi.SYNTH_PHASE, amplitude=-30000, add_re=-2768)
    assert plan_rc(t)[0] == -22 and "amplitude" in _err()


def test_tables_of_the_wrong_shape_are_refused():
    t = small_tables()
    assert plan_rc(t, ngain_sig=2)[0] == -22 and "signal gain table holds 2 entries, 1 classes x 3 SNRs need 3" in _err()
    assert plan_rc(t, ngain_sig=4)[0] == -22 and "gain table" in _err()
    assert plan_rc(t, nsnrs=0)[0] == -22 and "nsnrs must be in 1..64" in _err()
    assert plan_rc(t, nsnrs=65)[0] == -22 and "nsnrs" in _err()
    u = small_tables(first_point=1)
    assert plan_rc(u)[0] == -22 and "points 1 .. 2 lie outside the 2 points given" in _err()
    u = small_tables(first_tap=1)
    assert plan_rc(u)[0] == -22 and "taps 1 .. 4 lie outside the 4 taps given" in _err()
    u = small_tables()
    u["max_step"] = (1 << 30) + 1
    assert plan_rc(u)[0] == -22 and "max_step" in _err()
    for q in (0, 41):
        u = small_tables()
        u["q"] = q
        assert plan_rc(u)[0] == -22 and "q must be in 1..40" in _err()
    L = _cabi.lib()
    assert L.mdc_iq_synth_plan_bytes(0, 3, t["classes"].ctypes.data) == -22 and "nclasses" in _err()
    assert L.mdc_iq_synth_plan_bytes(1, 3, None) == -22 and "null classes" in _err()


def test_blob_size_mismatch_is_refused():
    t = small_tables()
    _, blob = plan_rc(t)
    for wrong in (blob.size - 16, blob.size + 16, 0):
        assert plan_rc(t, plan_bytes=wrong)[0] == -22 and f"plan_bytes is {wrong}, mdc_iq_synth_plan_bytes gives {blob.size}" in _err()


def test_plan_is_position_independent_and_frames_validates_it_before_any_device_call():
    L = _cabi.lib()
    blob = frontend.synth_plan(**small_tables())
    shifted = np.zeros(blob.size + 24, np.uint8)
    copy = shifted[8:8 + blob.size]
    copy[:] = blob                                                       # another address, another alignment class
    call = lambda p, nbytes, n, out=None: L.mdc_iq_synth_frames(p, None, nbytes, 1, 0, n, out, None, None, None, None)
    assert call(copy.ctypes.data, blob.size, 0) == 0                     # n_frames == 0: MDC_OK, nothing launched, buffers may be NULL
    assert call(copy.ctypes.data, blob.size, 1) == -22 and "null buffer" in _err()      # the plan itself passed
    assert call(copy.ctypes.data, blob.size - 16, 0) == -22 and "the plan holds" in _err()
    assert call(None, blob.size, 0) == -22 and "null plan" in _err()
    assert call(copy.ctypes.data, 8, 0) == -22 and "smaller than a plan's header" in _err()
    assert call(copy.ctypes.data, blob.size, -1) == -22 and "n_frames" in _err()
    assert call(copy.ctypes.data, blob.size, (1 << 30) + 1) == -22 and "n_frames" in _err()
    damaged = blob.copy()
    damaged[0] ^= 1
    assert call(damaged.ctypes.data, blob.size, 0) == -22 and "does not hold a plan" in _err()
    damaged = blob.copy()
    damaged[8] = 0                                                       # C = 0
    assert call(damaged.ctypes.data, blob.size, 0) == -22 and "header is damaged" in _err()
    buf = (ctypes.c_uint8 * 64)()
    assert call(copy.ctypes.data, blob.size, 1, ctypes.addressof(buf) + 2) == -22 and "4-byte aligned" in _err()


def test_unknown_modulation_is_refused_by_name():
    with pytest.raises(ValueError, match="'OFDM'"):
        frontend.synth_recipe(mods=("BPSK", "OFDM"))
    assert frontend.RML2016_MODS == ("8PSK", "AM-DSB", "AM-SSB", "BPSK", "CPFSK", "GFSK", "PAM4", "QAM16", "QAM64", "QPSK", "WBFM")


# ------------------------------------------------------------------------------------------------------------ 2. labels
@pytest.mark.parametrize("first", [0, 13, (1 << 32) + 3, (1 << 64) - 5])
def test_any_grid_of_consecutive_frames_holds_every_cell_once(first):
    C, S = 11, 20
    for offset in (0, 1, 57, 219):
        lab, snr = ref.labels_of(first + offset, C * S, C, S)
        if first + offset + C * S <= 1 << 64:          # (the raster restarts where the 64-bit index wraps: 2^64 is no multiple of C S)
            assert sorted(zip(lab.tolist(), snr.tolist())) == [(c, s) for c in range(C) for s in range(S)]
    lab, snr = ref.labels_of(first, 3, C, S)
    assert [(int(a), int(b)) for a, b in zip(lab, snr)] == [((first + i) % (C * S) % C, (first + i) % (C * S) // C) for i in range(3)]


# ------------------------------------------------------------------------------------------------------------ 3. statistics
@pytest.fixture(scope="module")
def recipe():
    return frontend.synth_recipe()


def one_class(recipe, k, gain_sig, gain_noise):
    """class k of a recipe as a one-class, one-SNR set of tables"""
    return dict(classes=recipe.classes[k:k + 1].copy(), points=recipe.points, taps=recipe.taps, gain_sig=np.array([[gain_sig]], np.int32),
                gain_noise=np.array([gain_noise], np.int32), max_step=recipe.max_step, q=recipe.q)


def within_five_standard_errors(per_frame, expected):
    mean, se = per_frame.mean(), per_frame.std(ddof=1) / np.sqrt(per_frame.size)
    assert abs(mean - expected) <= 5.0 * se, (mean, expected, se, (mean - expected) / se)


@pytest.mark.parametrize("k", range(11))
def test_signal_power_of_every_class_is_the_designs_exact_expectation(recipe, k):
    """g_noise = 0 and g_sig = 2^q: the output is the mixer's m itself (the final rounding changes nothing), whose expected power
    the design states exactly: the tables' exact second moments, plus 1/12 LSB^2 per component for each rounding on the way."""
    t = one_class(recipe, k, 1 << recipe.q, 0)
    iq, _, _, sat = ref.synth(seed=5, first_frame=0, n=64, **t)
    m, _, _, _ = ref.synth(seed=5, first_frame=0, n=FRAMES, stage="m", **t)
    assert sat == 0 and np.array_equal(iq.reshape(64, 128, 2), m[:64])
    per_frame = (m.astype(np.float64) ** 2).sum(axis=2).mean(axis=1)
    within_five_standard_errors(per_frame, recipe.power[k])
    assert frontend.synth_expected_power(recipe.classes[k], recipe.points, recipe.taps) == recipe.power[k]


def test_noise_variance_is_its_exact_rational(recipe):
    """g_sig = 0 and g_noise = 2^(q-4): out = (w + 8) >> 4, var(w) / 256 + 1/12 per component, var(w) = 8 (2^32 - 1) / 12."""
    t = one_class(recipe, 3, 0, 1 << (recipe.q - 4))
    iq, _, _, sat = ref.synth(seed=6, first_frame=0, n=FRAMES, **t)
    assert sat == 0
    num, den = ref.NOISE_VARIANCE
    assert frontend.SYNTH_NOISE_VARIANCE == num / den
    x = iq.astype(np.float64)
    within_five_standard_errors((x ** 2).mean(axis=1), num / den / 256.0 + 1.0 / 12.0)
    within_five_standard_errors(x.mean(axis=1), 0.0)
    assert np.abs(iq).max() <= (ref.GAUSS_MAX + 8) >> 4


@pytest.mark.parametrize("sps", [1, 3, 4, 8, 16])
def test_every_timing_offset_occurs(sps):
    tau = ref.timing_offsets(2016, ref.frame_indices(0, FRAMES), sps)
    assert sorted(set(tau.tolist())) == list(range(sps))


def test_carrier_step_stays_inside_its_range_and_reaches_both_halves(recipe):
    for max_step in (recipe.max_step, 1, 1 << 30):
        step = ref.carrier_steps(2016, ref.frame_indices(0, FRAMES), max_step)
        assert step.min() >= -max_step and step.max() <= max_step
        assert (step < 0).any() and (step > 0).any()
    assert (ref.carrier_steps(2016, ref.frame_indices(0, 64), 0) == 0).all()


@pytest.mark.parametrize("mod", LINEAR_MODS)
def test_in_band_power_share_of_the_linear_classes_is_the_pulses_own(recipe, mod):
    """The noise-free signal before the channel (z): the share of its power at |f| <= (1 + beta) / (2 sps), from 128-point
    periodograms of the frames, against the same share of the taps' own spectrum.  Symbols are independent and zero-mean and the
    timing offset is uniform, so z is stationary with autocorrelation r(t) = E|a|^2 / sps * sum_n h[n + t] conj(h[n]), and a
    rectangular frame's expected periodogram is sum_t r(t) (128 - |t|) e^{-2 pi i k t / 128}: |H(f)|^2 as the frame sees it.  A wrong
    polyphase branch order scrambles the pulse and spreads the power over the whole band."""
    k = recipe.mods.index(mod)
    c = recipe.classes[k]
    sps, span, beta = int(c["sps"]), int(c["span"]), 0.35
    h = recipe.taps[int(c["first_tap"]):int(c["first_tap"]) + sps * span].astype(np.float64)
    h = h[:, 0] + 1j * h[:, 1]
    r = np.correlate(h, h, mode="full")                      # lags -(T-1) .. T-1
    lags = np.arange(-(h.size - 1), h.size)
    kbin = np.arange(128)
    expected = (r[None, :] * (128 - np.abs(lags))[None, :] * np.exp(-2j * np.pi * kbin[:, None] * lags[None, :] / 128)).sum(axis=1).real
    f = np.fft.fftfreq(128)
    band = np.abs(f) <= (1 + beta) / (2 * sps)
    want = expected[band].sum() / expected.sum()
    assert 0.9 < want < 1.0          # (nearly all of it: what is missing is the rectangular frame's leakage and the truncated pulse)
    z, _, _, _ = ref.synth(seed=7, first_frame=0, n=FRAMES, stage="z", **one_class(recipe, k, 0, 0))
    Z = np.abs(np.fft.fft(z[:, :, 0] + 1j * z[:, :, 1], axis=1)) ** 2
    inband, total = Z[:, band].sum(axis=1), Z.sum(axis=1)
    share = inband.sum() / total.sum()
    se = (inband - share * total).std(ddof=1) / (np.sqrt(FRAMES) * total.mean())          # the ratio estimator's standard error
    assert abs(share - want) <= 5.0 * se, (share, want, se)
