"""Frame synthesis through the Rician multipath channel, on the host (no GPU): the fading restatement
(tests/iq_synth_fading_ref.py) against the unfaded one and against what a pure delay must give, mdc_iq_synth_frames_faded's
validation of the fading record through the C ABI, synth_fading's argument checks, and statistical checks of the restatement
against the design's exact expectations -- every statistical margin is 5 standard errors of the sample's own per-frame means,
plus, for the default channel, the in-band deviation the design itself reports.

Gains are Q13 (8192 is a gain of one; include/mdc.h says why not Q14), so the pure delay below has los = (8192, 0)."""
import numpy as np
import pytest

import iq_synth_fading_ref as fref
import iq_synth_ref as ref
from modulationdetectioncnn_amd import _cabi, frontend

FRAMES = 4096          # per statistical check
SEED = 2016
ONE = _cabi.SYNTH_FADING_GAIN_ONE


def _err():
    return _cabi.lib().mdc_last_error().decode()


def tables_of(r):
    return dict(classes=r.classes, points=r.points, taps=r.taps, gain_sig=r.gain_sig, gain_noise=r.gain_noise, max_step=r.max_step, q=r.q)


@pytest.fixture(scope="module")
def recipe():
    return frontend.synth_recipe()


@pytest.fixture(scope="module")
def default_fading():
    return frontend.synth_fading()


def one_class(recipe, k, gain_sig, gain_noise):
    return dict(classes=recipe.classes[k:k + 1].copy(), points=recipe.points, taps=recipe.taps, gain_sig=np.array([[gain_sig]], np.int32),
                gain_noise=np.array([gain_noise], np.int32), max_step=recipe.max_step, q=recipe.q)


# ------------------------------------------------------------------------------------------------ 1. the restatement itself
def test_without_a_head_the_new_restatement_gives_the_old_ones_mixed_samples(recipe):
    t = tables_of(recipe)
    unit = fref.fading_record([([16384], ONE, 0, 0)], 1)
    for first, n in ((0, 67), ((1 << 32) + 3, 23)):
        got = fref.synth(seed=SEED, first_frame=first, n=n, fading=unit, stage="m", **t)
        want = ref.synth(seed=SEED, first_frame=first, n=n, stage="m", **t)
        assert got[0].shape == (n, 128, 2)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    # ... and a unit channel (one tap of 16384, a gain of 8192) is the unfaded generator, down to the output bits
    got = fref.synth(seed=SEED, first_frame=5, n=67, fading=unit, **t)
    want = ref.synth(seed=SEED, first_frame=5, n=67, **t)
    assert np.array_equal(got[0], want[0]) and got[3] == want[3]


@pytest.mark.parametrize("mod", ["QAM16", "GFSK"])          # a LINEAR class and a PHASE class
@pytest.mark.parametrize("T", [2, 5, 16])
def test_a_delay_is_a_delay(recipe, mod, T):
    """One path, d = (0, 16384, 0, ...), a gain of exactly one, no Doppler: y_n is sample n + H - 1 of the H-headed stream."""
    k = recipe.mods.index(mod)
    assert int(recipe.classes[k]["mode"]) == (ref.PHASE if mod == "GFSK" else ref.LINEAR)
    t = one_class(recipe, k, 1 << recipe.q, 0)
    H = T - 1
    fading = fref.fading_record([([0, 16384] + [0] * (T - 2), ONE, 0, 0)], T)
    m = fref.synth(seed=SEED, first_frame=3, n=37, fading=fading, stage="m", **t)[0]
    y = fref.synth(seed=SEED, first_frame=3, n=37, fading=fading, stage="y", **t)[0]
    assert m.shape == (37, 128 + H, 2) and y.shape == (37, 128, 2)
    assert np.array_equal(y, m[:, H - 1:H - 1 + 128])
    assert np.abs(y).max() > 1000
    # the stream's first 128 samples do not depend on how long the head is (PHASE's running sum included)
    assert np.array_equal(m[:, :128], ref.synth(seed=SEED, first_frame=3, n=37, stage="m", **t)[0])
    # with g_sig = 2^q and no noise the output is y itself
    out = fref.synth(seed=SEED, first_frame=3, n=37, fading=fading, **t)
    assert out[3] == 0 and np.array_equal(out[0].reshape(37, 128, 2), y)


# ------------------------------------------------------------------------------------------------ 2. the record, through the C ABI
def small_plan():
    cl = np.zeros(1, _cabi.IQ_SYNTH_CLASS)
    cl[0]["source"], cl[0]["points"], cl[0]["sps"], cl[0]["span"], cl[0]["mode"] = _cabi.SYNTH_ALPHABET, 2, 2, 2, _cabi.SYNTH_LINEAR
    return frontend.synth_plan(cl, np.array([[1000, 0], [-1000, 0]], np.int16), np.array([[8000, 0], [4000, -100], [2000, 50], [1000, 0]], np.int16),
                               np.full((1, 3), 1 << 16, np.int32), np.full(3, 100, np.int32), 1 << 20, 16)


def valid_record():
    rec = np.zeros(1, _cabi.IQ_SYNTH_FADING)
    rec["paths"], rec["taps"] = 2, 3
    rec["path"][0][0]["delay_taps"][:3] = (100, 16000, -667)          # sums to 16767
    rec["path"][0][0]["los_re"], rec["path"][0][0]["los_im"], rec["path"][0][0]["scatter"] = 5000, -7000, 20000
    rec["path"][0][1]["delay_taps"][:3] = (0, 0, 16384)
    rec["path"][0][1]["scatter"] = 9000
    return rec


def faded_rc(rec, n=0):
    blob = np.ascontiguousarray(small_plan())
    ptr = None if rec is None else rec.ctypes.data
    return _cabi.lib().mdc_iq_synth_frames_faded(blob.ctypes.data, None, blob.size, 1, 0, n, None, None, None, None, ptr, None)


def test_a_valid_record_is_accepted_without_a_device():
    assert _cabi.IQ_SYNTH_PATH.itemsize == 48 and _cabi.IQ_SYNTH_FADING.itemsize == 208
    assert faded_rc(valid_record()) == 0, _err()
    assert faded_rc(valid_record(), n=1) == -22 and "mdc_iq_synth_frames_faded: null buffer" in _err()      # the record passed, then the plan
    assert faded_rc(None) == -22 and "null fading record" in _err()


@pytest.mark.parametrize("field,value,ok", [("paths", 0, False), ("paths", 5, False), ("paths", 1, False), ("paths", 2, True),
                                            ("taps", 0, False), ("taps", 17, False), ("taps", 16, True), ("taps", 2, False),
                                            ("max_doppler_step", 1 << 30, True), ("max_doppler_step", (1 << 30) + 1, False),
                                            ("reserved", 1, False), ("reserved", -1, False)])
def test_record_fields_at_and_past_their_limits(field, value, ok):
    """(paths = 1 leaves path 1 filled, taps = 2 leaves a third tap: both are fields that must then be 0)"""
    rec = valid_record()
    rec[field] = value
    rc = faded_rc(rec)
    assert rc == (0 if ok else -22), _err()
    if not ok:
        assert _err().startswith("mdc_iq_synth_frames_faded: fading:") and len(_err()) > 40


def test_path_preconditions_at_the_exact_bound():
    def with_path(p, **fields):
        rec = valid_record()
        for name, v in fields.items():
            if name == "taps":
                rec["path"][0][p]["delay_taps"][:len(v)] = v
            elif name.startswith("reserved"):
                rec["path"][0][p]["reserved"][int(name[-1])] = v
            else:
                rec["path"][0][p][name] = v
        return rec
    # sum |d| <= 32767
    assert faded_rc(with_path(0, taps=(-16383, 16000, 384))) == 0, _err()                       # 32767
    assert faded_rc(with_path(0, taps=(-16383, 16000, 385))) == -22 and "path 0: the delay taps sum to 32768" in _err()
    assert faded_rc(with_path(1, taps=(-32768, 0, 0))) == -22 and "path 1: the delay taps sum to 32768" in _err()
    # max(|los_re|, |los_im|) + scatter <= 32767
    assert faded_rc(with_path(0, los_re=5000, los_im=-12767, scatter=20000)) == 0, _err()       # 32767
    assert faded_rc(with_path(0, los_re=5000, los_im=-12768, scatter=20000)) == -22 and "path 0: max(|los_re|, |los_im|) + scatter" in _err()
    assert faded_rc(with_path(0, los_re=12768, los_im=0, scatter=20000)) == -22 and "12768 + 20000" in _err()
    assert faded_rc(with_path(1, los_re=0, los_im=0, scatter=32767)) == 0, _err()
    assert faded_rc(with_path(1, los_re=0, los_im=0, scatter=32768)) == -22 and "path 1" in _err()
    assert faded_rc(with_path(1, los_re=-32768, los_im=0, scatter=0)) == -22 and "32768 + 0" in _err()
    assert faded_rc(with_path(1, los_re=-32767, los_im=32767, scatter=0)) == 0, _err()
    assert faded_rc(with_path(0, scatter=0)) == 0, _err()
    assert faded_rc(with_path(0, scatter=-1)) == -22 and "scatter must be >= 0" in _err()
    # reserved fields, taps beyond `taps`, paths beyond `paths`
    assert faded_rc(with_path(0, reserved0=1)) == -22 and "path 0: reserved must be 0" in _err()
    assert faded_rc(with_path(1, reserved1=-5)) == -22 and "path 1: reserved must be 0" in _err()
    assert faded_rc(with_path(3, reserved1=2)) == -22 and "path 3: reserved must be 0" in _err()
    rec = valid_record()
    rec["path"][0][1]["delay_taps"][3] = 1
    assert faded_rc(rec) == -22 and "path 1: delay_taps[3] must be 0 with 3 taps" in _err()
    for name in ("los_re", "los_im", "scatter"):
        assert faded_rc(with_path(2, **{name: 1})) == -22 and "path 2: every field of a path beyond the 2 in use must be 0" in _err()
    assert faded_rc(with_path(3, taps=(0, 1, 0))) == -22 and "path 3" in _err()


def test_the_plan_is_still_checked():
    blob = np.ascontiguousarray(small_plan())
    rec = valid_record()
    L = _cabi.lib()
    assert L.mdc_iq_synth_frames_faded(blob.ctypes.data, None, blob.size - 16, 1, 0, 0, None, None, None, None, rec.ctypes.data, None) == -22
    assert "mdc_iq_synth_frames_faded: plan_bytes" in _err()
    assert L.mdc_iq_synth_frames_faded(None, None, blob.size, 1, 0, 0, None, None, None, None, rec.ctypes.data, None) == -22 and "null plan" in _err()


# ------------------------------------------------------------------------------------------------ 3. the designer
def test_default_design(default_fading):
    f = default_fading
    rec = f.record.reshape(-1)[0]
    assert faded_rc(f.record) == 0, _err()
    assert (int(rec["paths"]), int(rec["taps"]), int(rec["max_doppler_step"])) == (3, 8, 0)
    assert int(rec["path"][0]["los_re"]) > 0 and all(int(rec["path"][p]["los_re"]) == 0 for p in (1, 2, 3))      # line of sight on path 0 only
    assert abs(f.power_sum - 1.0) < 1e-3 and abs(sum(f.path_power) - f.power_sum) < 1e-12
    # the reported powers are the integer definition's: recomputed here from the record alone
    for p in range(3):
        path = rec["path"][p]
        assert f.path_power[p] == frontend.synth_path_power(int(path["los_re"]), int(path["los_im"]), int(path["scatter"])) / ONE ** 2
    share = np.array(f.mags) ** 2 / np.sum(np.array(f.mags) ** 2)
    assert np.allclose(f.path_power, share, rtol=1e-3)
    k_got = float(rec["path"][0]["los_re"]) ** 2 / (f.path_power[0] * ONE ** 2 - float(rec["path"][0]["los_re"]) ** 2)
    assert abs(k_got - 4.0) < 0.01
    assert len(f.delay_deviation) == 3 and all(0.0 < d < 0.05 for d in f.delay_deviation)
    # every delay filter has unit gain at DC up to its rounding, and its centre of mass sits where the delay puts it
    for p in range(3):
        d = rec["path"][p]["delay_taps"].astype(np.float64)
        assert abs(d.sum() - 16384) <= 4 and (d[8:] == 0).all()
        assert abs((d * np.arange(16)).sum() / d.sum() - (3.5 + f.delays[p])) < 0.05


def test_scatter_moments_are_those_of_the_integer_definition():
    m1, m2 = frontend.synth_scatter_moments(0)
    assert m1 == 0.0 and m2 == 0.0
    # scatter = 2^18: X = G exactly
    m1, m2 = frontend.synth_scatter_moments(1 << 18)
    num, den = ref.NOISE_VARIANCE
    assert abs(m1) < 1e-6 and abs(m2 / (num / den) - 1.0) < 1e-12
    # a sampled check of a mid-sized scatter, against the draws themselves
    g = ref.gauss(ref.frame_keys(1, np.arange(1 << 16, dtype=np.uint64)), np.uint64(768))
    x = ((g * 9000 + (1 << 17)) >> 18).astype(np.float64)
    m1, m2 = frontend.synth_scatter_moments(9000)
    assert abs(x.mean() - m1) <= 5.0 * x.std(ddof=1) / 256.0
    assert abs((x ** 2).mean() - m2) <= 5.0 * (x ** 2).std(ddof=1) / 256.0


@pytest.mark.parametrize("kwargs,text", [(dict(delays=()), "delays"), (dict(delays=(0,) * 5, mags=(1,) * 5), "delays"),
                                         (dict(mags=(1.0, 0.5)), "mags"), (dict(mags=(1.0, 0.0, 0.3)), "mags"), (dict(mags=(1.0, -1.0, 0.3)), "mags"),
                                         (dict(ntaps=0), "ntaps"), (dict(ntaps=17), "ntaps"), (dict(delays=(0.0, 0.9, 3.6)), "delays"),
                                         (dict(delays=(-0.1, 0.9, 1.7)), "delays"), (dict(rician_k=-1.0), "rician_k"),
                                         (dict(rician_k=float("nan")), "rician_k"), (dict(max_doppler=0.3), "max_doppler"),
                                         (dict(max_doppler=-0.01), "max_doppler"), (dict(band=0.0), "band")])
def test_bad_designs_are_refused_by_name(kwargs, text):
    with pytest.raises(ValueError, match=text):
        frontend.synth_fading(**kwargs)


def test_extreme_designs_pass_the_librarys_own_check():
    for kwargs in (dict(delays=(0.0,), mags=(1.0,), rician_k=0.0, ntaps=1), dict(delays=(0.0,), mags=(2.0,), rician_k=1e6, ntaps=1),
                   dict(delays=(0.0, 0.5, 1.0, 1.5), mags=(1.0, 1.0, 1.0, 1.0), ntaps=16, max_doppler=0.25, kaiser_beta=8.0), dict(rician_k=0.0)):
        f = frontend.synth_fading(**kwargs)
        assert faded_rc(f.record) == 0, (kwargs, _err())
        assert abs(f.power_sum - 1.0) < 1e-3
    # sixteen taps of a half-sample sinc under the default window sum to more than 2 in absolute value: the record's precondition
    with pytest.raises(ValueError, match="path 0's delay filter sums to"):
        frontend.synth_fading(delays=(0.0,), mags=(1.0,), ntaps=16)


def test_the_recipe_carries_the_design_and_nothing_else_changes(recipe, default_fading):
    r = frontend.synth_recipe(fading=default_fading)
    assert r.fading is default_fading and recipe.fading is None
    assert r.blob.tobytes() == recipe.blob.tobytes() and np.array_equal(r.gain_sig, recipe.gain_sig)
    with pytest.raises(TypeError, match="SynthFading"):
        frontend.synth_recipe(fading=default_fading.record)


# ------------------------------------------------------------------------------------------------ 4. statistics
def within_five_standard_errors(per_frame, expected):
    mean, se = per_frame.mean(), per_frame.std(ddof=1) / np.sqrt(per_frame.size)
    assert abs(mean - expected) <= 5.0 * se, (mean, expected, se, (mean - expected) / se)


@pytest.mark.parametrize("max_doppler_step", [0, 1 << 24])
def test_gain_statistics_of_one_flat_path(max_doppler_step):
    """A one-point alphabet through a one-tap pulse is a constant: m is that constant through the mixer, u = m (P = 1, T = 1,
    d = 16384), and y = r m / 8192.  g, the Doppler phase and the mixer phase are independent draws, so
        E|y|^2 = E|r|^2 E|m|^2 / 2^26 + 1/6,   E|r|^2 = E|g|^2 (Doppler off)  or  E|g|^2 mean(c^2 + s^2) / 2^30 + 1/6 (on),
    E|g|^2 = |los|^2 + 2 E X^2 + 2 E X (los_re + los_im) summed over the drawn integer's whole distribution
    (synth_path_power), E|m|^2 as synth_expected_power states it; each rounding shift adds 1/12 per component."""
    cl = np.zeros(1, _cabi.IQ_SYNTH_CLASS)
    cl[0]["source"], cl[0]["points"], cl[0]["sps"], cl[0]["span"], cl[0]["mode"] = ref.ALPHABET, 1, 1, 1, ref.LINEAR
    points, taps = np.array([[16384, 0]], np.int16), np.array([[32767, 0]], np.int16)
    q = 12
    t = dict(classes=cl, points=points, taps=taps, gain_sig=np.array([[1 << q]], np.int32), gain_noise=np.array([0], np.int32), max_step=1 << 26, q=q)
    los, scatter = (3000, -2000), 9000
    fading = fref.fading_record([([16384], los[0], los[1], scatter)], 1, max_doppler_step)
    y = fref.synth(seed=9, first_frame=0, n=FRAMES, fading=fading, stage="y", **t)[0]
    per_frame = (y.astype(np.float64) ** 2).sum(axis=2).mean(axis=1)
    table = fref._TABLE.astype(np.float64)
    e_g = frontend.synth_path_power(los[0], los[1], scatter)
    m1, m2 = frontend.synth_scatter_moments(scatter)
    assert abs(e_g - (los[0] ** 2 + los[1] ** 2 + 2.0 * (m2 - m1 * m1))) < 1e-3 * e_g          # |los|^2 + 2 Var(X), up to E X
    e_r = e_g if max_doppler_step == 0 else e_g * float(np.mean((table ** 2).sum(axis=1))) / 2.0 ** 30 + 1.0 / 6.0
    e_m = frontend.synth_expected_power(cl[0], points, taps)
    within_five_standard_errors(per_frame, e_r * e_m / 2.0 ** 26 + 1.0 / 6.0)
    if max_doppler_step == 0:          # without Doppler the gain is one number per frame: |y|^2 hardly moves inside a frame
        assert (np.ptp((y.astype(np.float64) ** 2).sum(axis=2), axis=1) <= 0.01 * per_frame + 200).all()
    else:
        ph = np.unwrap(np.angle(y[:, :, 0] + 1j * y[:, :, 1]), axis=1)
        assert (ph[:, -1] - ph[:, 0] > 0).any() and (ph[:, -1] - ph[:, 0] < 0).any()          # both signs of nu occur (the mixer's step too)


@pytest.mark.parametrize("k", range(11))
def test_mean_power_after_the_default_channel(recipe, default_fading, k):
    """Every class of the default recipe at 18 dB: mean power of the faded frames over mean power of the same frames unfaded.  The
    paths' gains are independent and only path 0 has a constant part, so the cross terms vanish in expectation and the ratio is
    sum_p E|g_p|^2 (one by design: power_sum) times each delay filter's power gain over the signal's band -- within the worst
    in-band deviation the design reports, plus 5 standard errors of the ratio estimator.  Measured ratios: DESIGN.md 5.26."""
    s18 = recipe.snrs_db.index(18)
    t = one_class(recipe, k, int(recipe.gain_sig[k, s18]), int(recipe.gain_noise[s18]))
    fading = fref.record_of(default_fading.record)
    faded, _, _, sat_f = fref.synth(seed=12, first_frame=0, n=FRAMES, fading=fading, **t)
    plain, _, _, sat_p = ref.synth(seed=12, first_frame=0, n=FRAMES, **t)
    pf, pp = (faded.astype(np.float64) ** 2).mean(axis=1), (plain.astype(np.float64) ** 2).mean(axis=1)
    ratio = pf.mean() / pp.mean()
    se = (pf - ratio * pp).std(ddof=1) / (np.sqrt(FRAMES) * pp.mean())
    bound = max(default_fading.delay_deviation) + 5.0 * se
    print(f"{recipe.mods[k]}: ratio {ratio:.4f}, standard error {se:.4f}, deviation {max(default_fading.delay_deviation):.4f}, saturated {sat_f}/{sat_p}")
    assert abs(default_fading.power_sum - 1.0) < 1e-3
    assert abs(ratio - 1.0) <= bound, (recipe.mods[k], ratio, se, bound)
