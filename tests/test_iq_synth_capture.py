"""mdc_iq_synth_scene / mdc_iq_synth_scene_hops and the scene design, truth and scoring of frontend.py, without a GPU: the host
entry points against the numpy restatement (tests/iq_synth_capture_ref.py), and the restatement against the design."""
import numpy as np
import pytest

import iq_synth_capture_cases as K
import iq_synth_capture_ref as R
from modulationdetectioncnn_amd import _cabi, frontend as F


def _one(**kw):
    """one valid QPSK record on the single tap 32767"""
    em = np.zeros(1, _cabi.IQ_SYNTH_EMITTER)
    em["cls"], em["interpolate"], em["decimate"], em["first_tap"], em["ntaps"], em["gain"], em["hops"] = 0, 1, 1, 0, 1, 1000, 1
    for k, v in kw.items():
        em[k] = v
    return em


def _refused(emitters, taps, text, **kw):
    with pytest.raises(_cabi.MdcError) as e:
        F.synth_scene_blob(K.recipe().blob, emitters, np.asarray(taps, np.int16), kw.get("gain_noise", 0), kw.get("q", 20), (0, 0))
    assert e.value.code == -22          # MDC_EINVAL
    assert text in str(e.value), str(e.value)


@pytest.mark.parametrize("change, taps, text", [
    (dict(cls=len(K.MODS)), [32767], "emitter 1: cls"),
    (dict(cls=-1), [32767], "emitter 1: cls"),
    (dict(interpolate=0), [32767], "emitter 1: interpolate"),
    (dict(interpolate=33, decimate=1), [32767], "emitter 1: interpolate"),
    (dict(decimate=0), [32767], "emitter 1: decimate"),
    (dict(interpolate=2, decimate=3), [32767], "emitter 1: decimate"),
    (dict(ntaps=3), [32767, 32767, 2], "emitter 1: the taps of branch 0"),
    (dict(ntaps=65), [1] * 65, "emitter 1: a branch holds"),
    (dict(ntaps=2), [32767], "emitter 1: taps"),
    (dict(ntaps=0), [32767], "emitter 1: ntaps"),
    (dict(hops=2, period=0), [32767], "emitter 1: 2 hops need a period"),
    (dict(hops=9, period=5), [32767], "emitter 1: hops"),
    (dict(reserved=(0, 1)), [32767], "emitter 1: reserved"),
    (dict(start=-1), [32767], "emitter 1: start"),
])
def test_every_refusal_names_its_emitter(change, taps, text):
    """the bad record is the SECOND of two, so the name in the text is the record's index and not a constant"""
    _refused(np.concatenate([_one(), _one(**change)]), taps, text)


def test_more_than_32_emitters_are_refused_by_name():
    _refused(np.concatenate([_one()] * 33), [32767], "emitter 32")
    assert _cabi.lib().mdc_iq_synth_scene_bytes(33, 1) == -22


def test_scalars_are_refused():
    _refused(_one(), [32767], "gain_noise", gain_noise=-1)
    _refused(_one(), [32767], "q must be", q=41)


def test_design_resampler_output_is_accepted_as_it_is():
    r = K.recipe()
    for L, D in ((2, 1), (3, 2), (32, 31), (32, 1), (7, 5)):
        h = F.design_resampler(L, D)
        em = _one(interpolate=L, decimate=D, ntaps=h.size)
        assert F.synth_scene_blob(r.blob, em, h, 0, 20).size > 0
    h = F.design_resampler(32, 1, ntaps=1024)
    assert F.synth_scene_blob(r.blob, _one(interpolate=32, ntaps=1024), h, 0, 20).size > 0


def test_same_inputs_same_blob_bytes():
    a, b = K._cases()["hopper_8"], K._cases()["hopper_8"]
    assert a.blob.tobytes() == b.blob.tobytes()
    assert a.blob.size == _cabi.lib().mdc_iq_synth_scene_bytes(a.emitters.size, a.taps.size)


def test_scene_hops_equal_the_restatements_draws():
    s = K.cases()["hopper_8"]
    for e, hops in ((0, 8), (1, 3)):
        for first in (0, 5, 1 << 33):
            got = F.synth_scene_hops(s, 77, e, first, 300)
            want = R.hop_indices(77, e, np.arange(first, first + 300, dtype=np.uint64), hops)
            assert np.array_equal(got, want)
    assert len(set(F.synth_scene_hops(s, 77, 0, 0, 300).tolist())) == 8
    with pytest.raises(_cabi.MdcError):
        F.synth_scene_hops(s, 77, 2, 0, 1)


@pytest.mark.parametrize("name", K.CASE_NAMES)
def test_cases_run_through_the_restatement_and_do_what_they_say(name):
    """every bound the header proves is asserted inside the restatement; the clamp cases clamp"""
    out, sat = R.scene_capture(K.cases()[name], K.SEED, K.LENGTHS[0])
    assert out.shape == (K.LENGTHS[0], 2)
    assert (sat > 0) == (name in K.MUST_SATURATE)
    if name == "nothing":
        assert not out.any()


def test_synth_scene_refuses_bad_arguments_by_name():
    r = K.recipe()
    ok = dict(mod="QPSK", samples_per_symbol=16, centre=0.1, rms=100.0)
    for change, text in ((dict(mod="OOK"), "emitter 0: mod"), (dict(samples_per_symbol=4), "emitter 0: samples_per_symbol"),
                         (dict(centre=0.7), "emitter 0: centre"), (dict(centre=[0.1, 0.2]), "emitter 0: a hopper"),
                         (dict(level_db=3.0), "emitter 0: give level_db or rms"), (dict(start=-3), "emitter 0: start"),
                         (dict(colour="red"), "emitter 0: unknown key"), (dict(interpolate=2), "emitter 0: give samples_per_symbol or")):
        with pytest.raises(ValueError, match=text):
            F.synth_scene(r, [dict(ok, **change)], 10.0)
    with pytest.raises(ValueError, match="at most 32"):
        F.synth_scene(r, [ok] * 33, 10.0)
    with pytest.raises(ValueError, match="emitter 0: level_db is relative"):
        F.synth_scene(r, [dict(mod="QPSK", samples_per_symbol=16, level_db=10.0)], 0.0)
    s = F.synth_scene(r, [ok, dict(ok, centre=-0.2)], 10.0)
    assert s.taps.size == F.design_resampler(2, 1).size          # equal filters are stored once
    assert (s.emitters["interpolate"] == 2).all() and (s.emitters["decimate"] == 1).all()


def _signal_only(em):
    return F.synth_scene(K.recipe(), [em], 0.0)


@pytest.mark.parametrize("em", [dict(mod="QPSK", samples_per_symbol=16, centre=0.125, rms=3000.0),
                                dict(mod="GFSK", interpolate=3, decimate=2, centre=-0.3, rms=2000.0),
                                dict(mod="AM-DSB", interpolate=1, decimate=1, centre=0.2, rms=2500.0),
                                dict(mod="8PSK", interpolate=32, decimate=31, centre=-0.0625, rms=1500.0)], ids=lambda e: e["mod"])
def test_restatement_meets_the_design_power_and_centre(em):
    """Signal only: the mean power is within 5 standard errors (of the mean of 64 block means) of the scene's exact expectation,
    widened by the reported passband deviation; the periodogram's centroid sits at the designed centre to within one bin."""
    s = _signal_only(em)
    n = 1 << 16
    out, sat = R.scene_capture(s, 11, n)
    assert sat == 0
    x = out[:, 0].astype(np.float64) + 1j * out[:, 1].astype(np.float64)
    p = np.abs(x) ** 2
    blocks = p.reshape(64, -1).mean(axis=1)
    mean, se = blocks.mean(), blocks.std(ddof=1) / np.sqrt(blocks.size)
    want = s.rms[0] ** 2
    print(f"{em['mod']}: mean power {mean:.1f}, designed {want:.1f}, standard error {se:.1f}, passband deviation {s.passband_deviation[0]:.2e}")
    assert abs(mean - want) <= 5.0 * se + s.passband_deviation[0] * want + 1.0          # + 1: the output rounding's 2 / 12 and slack of one LSB^2
    nfft = 1024
    psd = (np.abs(np.fft.fft(x.reshape(-1, nfft) * np.hanning(nfft)[None, :], axis=1)) ** 2).mean(axis=0)
    f = np.fft.fftfreq(nfft)
    rel = (f - em["centre"] + 0.5) % 1.0 - 0.5          # frequencies relative to the designed centre
    centroid = float(np.sum(rel * psd) / psd.sum())
    print(f"{em['mod']}: centroid {centroid * nfft:+.3f} bins off the designed centre")
    assert abs(centroid) <= 1.0 / nfft


def test_truth_outside_the_widened_intervals_is_exactly_dc():
    r = K.recipe()
    s = F.synth_scene(r, [dict(mod="BPSK", samples_per_symbol=16, centre=0.1, rms=3000.0, start=3000, on=2500, period=9000),
                          dict(mod="GFSK", interpolate=3, decimate=2, centre=[-0.3, -0.1, 0.3], rms=2000.0, start=1000, on=1500, period=4000),
                          dict(mod="QPSK", samples_per_symbol=8, centre=-0.4, rms=1000.0, start=20000, on=700)], 0.0, dc=(5, -7))
    n = 30000
    out, _ = R.scene_capture(s, 3, n)
    truth = F.scene_truth(s, n, 3)
    assert set(truth["emitter"].tolist()) == {0, 1, 2}
    quiet = np.ones(n, bool)
    for row in truth:
        em = s.emitters[row["emitter"]]
        c = r.classes[em["cls"]]
        L, D = int(em["interpolate"]), int(em["decimate"])
        reach = -(-(int(em["ntaps"]) + int(c["sps"]) * int(c["span"]) * L) // D) + 2          # the filter's and the pulse's lengths, in capture pairs
        quiet[max(row["first_pair"] - reach, 0):row["stop_pair"] + reach] = False
    assert quiet.sum() > n // 4
    assert (out[quiet] == np.array([5, -7])).all()
    # and inside its interval every dwell carries power, at the truth's centre
    for row in truth:
        seg = out[row["first_pair"]:row["stop_pair"]].astype(np.float64) - np.array([5.0, -7.0])
        assert (seg ** 2).sum(axis=1).mean() > 0.5 * s.rms[row["emitter"]] ** 2
    hopper = truth[truth["emitter"] == 1]
    assert len(hopper) >= 6 and len(set(hopper["centre"].tolist())) > 1
    assert np.array_equal(np.array([s.centres[1].index(c) for c in hopper["centre"]]), F.synth_scene_hops(s, 3, 1, 0, len(hopper)))
    x = out[:, 0] + 1j * out[:, 1].astype(np.float64)
    for row in hopper:
        seg = x[row["first_pair"]:row["stop_pair"]][:1024]
        psd, f = np.abs(np.fft.fft(seg * np.hanning(seg.size))) ** 2, np.fft.fftfreq(seg.size)
        band = [psd[np.abs((f - c + 0.5) % 1.0 - 0.5) <= row["bandwidth"] / 2.0].sum() for c in s.centres[1]]          # (the other emitters lie outside all three)
        assert s.centres[1][int(np.argmax(band))] == row["centre"]


def test_prefix_property_in_the_restatement():
    for name in ("gauss_and_phase_continuous", "burst_edges", "hopper_8"):
        s = K.cases()[name]
        long, _ = R.scene_capture(s, 5, 3149)
        short, _ = R.scene_capture(s, 5, 1500)
        assert np.array_equal(long[:1500], short)


def test_an_emitters_contribution_is_additive():
    """m_{e,n} depends on the emitter's own record and index alone, and the output is the stated sum of the stages"""
    s = K.cases()["burst_edges"]
    n = 2125
    mixed, _ = R.scene_capture(s, 9, n, stage="m")
    for e in range(len(s.emitters)):
        others = s.emitters.copy()
        others["gain"] = 0
        for k in range(len(others)):          # every other slot holds a different emitter
            if k != e:
                others[k] = s.emitters[(k + 1) % len(others) if (k + 1) % len(others) != e else e]
        alone, _ = R.capture(s.recipe.classes, s.recipe.points, s.recipe.taps, others, s.taps, s.gain_noise, s.q, s.dc, 9, n, stage="m")
        assert np.array_equal(alone[e], mixed[e])
    out, sat = R.scene_capture(s, 9, n)
    v = (mixed * s.emitters["gain"].astype(np.int64)[:, None, None]).sum(axis=0) + R.noise(9, n) * s.gain_noise + (1 << (s.q - 1))
    assert np.array_equal(out, np.clip((v >> s.q) + np.array(s.dc), -32768, 32767).astype(np.int16))


def test_end_to_end_scene_meets_its_conditions_under_the_numpy_references():
    """the scene of the GPU suite's end-to-end test, on the restatement: the numpy references of the spectrogram, the threshold
    rule and the components find every whole dwell of at least three rows and nothing else"""
    scene = K.e2e_scene()
    assert min(scene.level_db) >= 15.0
    out, sat = R.scene_capture(scene, K.SEED, K.E2E_PAIRS)
    truth = F.scene_truth(scene, K.E2E_PAIRS, K.SEED)
    must = K.e2e_must_find(truth)
    assert sat == 0 and len(truth) == 14 and len(must) == 13
    assert {(int(t["emitter"]), round(float(t["centre"]), 2)) for t in truth} >= {(0, -0.35), (1, -0.15), (3, 0.45), (4, 0.45)}
    assert len({float(t["centre"]) for t in truth[truth["emitter"] == 2]}) >= 3          # the hopper visits several carriers
    recs = K.numpy_detections(out)
    assert min(r["snr_db"] for r in recs) >= 15.0
    score = F.score_detections(recs, truth)
    assert not set(must) & set(score["missed"]) and score["false"] == []


def test_score_detections_counts_found_missed_false_and_labels():
    truth = np.array([(0, "QPSK", 0, 0, 1000, 5000, 0.10, 0.05, 20.0, True), (1, "BPSK", 1, 0, 8000, 9000, -0.2, 0.04, 20.0, True),
                      (1, "BPSK", 1, 1, 12000, 13000, -0.2, 0.04, 20.0, True)], dtype=F.SCENE_TRUTH)
    recs = [dict(first_pair=900, stop_pair=4000, centre=0.11, label=0),          # finds dwell 0 (3000 of 4000 pairs)
            dict(first_pair=8000, stop_pair=8400, centre=-0.2, label=1),         # 40 % of dwell 1: not enough
            dict(first_pair=12000, stop_pair=13000, centre=0.3, label=1),        # right time, wrong band
            dict(first_pair=11900, stop_pair=13100, centre=-0.21, label=0)]      # finds dwell 2, mislabelled
    s = F.score_detections(recs, truth, min_overlap=0.5, classes=2)
    assert s["found"] == [(0, 0), (2, 3)] and s["missed"] == [1] and s["false"] == [1, 2]
    assert s["confusion"].tolist() == [[1, 0], [1, 0]] and s["accuracy"] == 0.5
    assert F.score_detections(recs, truth, min_overlap=0.4, classes=2)["missed"] == []
    empty = F.score_detections([], truth)
    assert empty["missed"] == [0, 1, 2] and empty["false"] == [] and np.isnan(empty["accuracy"])
