"""The scenes tests/test_iq_synth_capture_gpu.py holds mdc_iq_synth_capture to bit for bit, one per path the kernel can take, and
the end-to-end scene.  Built on the host only; tests/test_iq_synth_capture.py runs the restatement over every one of them, so a
case that does not exercise what its name says (a clamp that never clamps) fails without a GPU."""
import numpy as np

from modulationdetectioncnn_amd import _cabi, frontend as F

LENGTHS = (2 * 1024 + 77, 3 * 1024)          # a tile tail; interior tile seams only
MODS = ("QPSK", "BPSK", "GFSK", "AM-DSB", "8PSK", "CPFSK", "WBFM")

_recipes = {}


def recipe(sps=8):
    if sps not in _recipes:
        mods = MODS if sps == 8 else ("QPSK", "GFSK")
        _recipes[sps] = F.synth_recipe(mods=mods, snrs_db=(10,), sps=sps, span=8)
    return _recipes[sps]


def raw(scene, emitters=None, taps=None, gain_noise=None, q=None, dc=None):
    """the scene with records, taps or scalars replaced as given, its blob rebuilt by mdc_iq_synth_scene"""
    emitters = scene.emitters if emitters is None else emitters
    taps = scene.taps if taps is None else np.asarray(taps, np.int16)
    gain_noise = scene.gain_noise if gain_noise is None else gain_noise
    q = scene.q if q is None else q
    dc = scene.dc if dc is None else dc
    blob = F.synth_scene_blob(scene.recipe.blob, emitters, taps, gain_noise, q, dc)
    return scene._replace(emitters=emitters, taps=taps, gain_noise=gain_noise, q=q, dc=dc, blob=blob)


def _with_filter(scene, k, L, D, h):
    """emitter k on the filter h at L / D (h appended to the scene's taps)"""
    em = scene.emitters.copy()
    em[k]["interpolate"], em[k]["decimate"], em[k]["first_tap"], em[k]["ntaps"] = L, D, scene.taps.size, len(h)
    return raw(scene, emitters=em, taps=np.concatenate([scene.taps, np.asarray(h, np.int16)]))


def _cases():
    r = recipe()
    c = {}
    c["L1_D1_T1"] = F.synth_scene(r, [dict(mod="QPSK", interpolate=1, decimate=1, centre=0.11, rms=3000.0)], 200.0)
    c["L3_D2"] = F.synth_scene(r, [dict(mod="8PSK", interpolate=3, decimate=2, centre=-0.2, rms=3000.0, phase0=12345)], 200.0)
    s = F.synth_scene(r, [dict(mod="QPSK", interpolate=32, decimate=1, centre=0.3, rms=3000.0)], 200.0)
    c["L32_D1_T1024"] = _with_filter(s, 0, 32, 1, F.design_resampler(32, 1, ntaps=1024))
    c["L32_D31"] = F.synth_scene(r, [dict(mod="BPSK", interpolate=32, decimate=31, centre=0.05, rms=3000.0)], 200.0)
    c["gauss_and_phase_continuous"] = F.synth_scene(r, [dict(mod="AM-DSB", interpolate=2, decimate=1, centre=0.25, rms=2500.0),
                                                        dict(mod="GFSK", interpolate=3, decimate=2, centre=-0.3, rms=2500.0),
                                                        dict(mod="WBFM", interpolate=1, decimate=1, centre=-0.05, rms=2000.0),
                                                        dict(mod="CPFSK", interpolate=5, decimate=4, centre=0.4, rms=2000.0)], 150.0)
    # on for the first tile and the last, off for the whole tile(s) between: the phase still advances
    c["phase_gated_off_mid_tile"] = F.synth_scene(r, [dict(mod="GFSK", interpolate=2, decimate=1, centre=0.1, rms=3000.0, start=0, on=700,
                                                           period=2300)], 100.0)
    c["burst_edges"] = F.synth_scene(r, [dict(mod="BPSK", interpolate=2, decimate=1, centre=0.1, rms=3000.0, start=300, on=411, period=1500),
                                         dict(mod="QPSK", interpolate=3, decimate=2, centre=-0.2, rms=3000.0, start=17, on=90, period=200),
                                         dict(mod="8PSK", interpolate=2, decimate=1, centre=0.3, rms=2000.0, start=100, on=640, period=640),
                                         dict(mod="GFSK", interpolate=1, decimate=1, centre=-0.4, rms=2000.0, start=50, on=5, period=7),
                                         dict(mod="QPSK", interpolate=2, decimate=1, centre=0.45, rms=3000.0, start=10 ** 6),
                                         dict(mod="BPSK", interpolate=2, decimate=1, centre=-0.45, rms=3000.0, start=1500, on=400)], 100.0)
    c["hopper_8"] = F.synth_scene(r, [dict(mod="GFSK", interpolate=2, decimate=1, centre=[-0.4, -0.3, -0.2, -0.1, 0.1, 0.2, 0.3, 0.4],
                                           rms=3000.0, start=40, on=500, period=600),
                                      dict(mod="QPSK", interpolate=3, decimate=2, centre=[0.0, 0.25, -0.25], rms=2000.0, on=90, period=100)], 100.0)
    c["sps1"] = F.synth_scene(recipe(1), [dict(mod="QPSK", interpolate=4, decimate=3, centre=0.1, rms=3000.0),
                                          dict(mod="GFSK", interpolate=1, decimate=1, centre=-0.2, rms=2000.0, start=100, on=900, period=1000)], 100.0)
    c["sps16"] = F.synth_scene(recipe(16), [dict(mod="QPSK", interpolate=5, decimate=4, centre=0.1, rms=3000.0),
                                            dict(mod="GFSK", interpolate=2, decimate=1, centre=-0.2, rms=2000.0)], 100.0)
    c["E0"] = F.synth_scene(r, [], 300.0)
    ems = [dict(mod=MODS[k % len(MODS)], interpolate=1 + k % 5, decimate=1 + k % (1 + k % 5), centre=(k - 16) / 34.0, rms=400.0,
                start=37 * k, on=1900 + k, period=(2000 + 3 * k) if k % 3 else 0) for k in range(32)]
    c["E32"] = F.synth_scene(r, ems, 100.0)
    c["no_noise"] = F.synth_scene(r, [dict(mod="QPSK", interpolate=2, decimate=1, centre=0.1, rms=3000.0)], 0.0)
    c["nothing"] = F.synth_scene(r, [], 0.0, dc=(0, 0))
    c["dc"] = F.synth_scene(r, [dict(mod="BPSK", interpolate=2, decimate=1, centre=0.1, rms=1000.0, start=500, on=800)], 50.0, dc=(-321, 1234))
    c["output_clamp"] = F.synth_scene(r, [dict(mod="QPSK", interpolate=2, decimate=1, centre=0.1, rms=30000.0)], 3000.0)
    s = F.synth_scene(r, [dict(mod="AM-DSB", interpolate=1, decimate=1, centre=0.1, rms=3000.0)], 100.0)
    c["interpolation_clamp"] = _with_filter(s, 0, 1, 1, [32767, 32767])          # twice the signal: the carrier plus message passes 32767
    return c


_built = None


def cases():
    global _built
    if _built is None:
        _built = _cases()
    return _built


CASE_NAMES = ("L1_D1_T1", "L3_D2", "L32_D1_T1024", "L32_D31", "gauss_and_phase_continuous", "phase_gated_off_mid_tile", "burst_edges", "hopper_8",
              "sps1", "sps16", "E0", "E32", "no_noise", "nothing", "dc", "output_clamp", "interpolation_clamp")
MUST_SATURATE = ("output_clamp", "interpolation_clamp")
SEED = 2016


# ---- the end-to-end scene: 2^19 pairs -------------------------------------------------------------------------------------------------
E2E_PAIRS = 1 << 19
E2E_NFFT, E2E_AVG = 1024, 8


def e2e_scene():
    """A continuous QPSK, a bursty BPSK, a GFSK hopper over four carriers, and two emitters that share bins at different times;
    levels >= 15 dB above the floor inside each emitter's band."""
    r = recipe()
    row = E2E_NFFT // 2 * E2E_AVG          # capture pairs per spectrogram row
    return F.synth_scene(r, [
        dict(mod="QPSK", samples_per_symbol=32, centre=-0.35, level_db=20.0),
        dict(mod="BPSK", samples_per_symbol=32, centre=-0.15, level_db=20.0, start=10 * row, on=20 * row, period=40 * row),
        dict(mod="GFSK", samples_per_symbol=32, centre=[0.05, 0.15, 0.25, 0.35], level_db=20.0, start=4 * row, on=12 * row, period=16 * row),
        dict(mod="8PSK", samples_per_symbol=32, centre=0.45, level_db=20.0, start=8 * row, on=24 * row),
        dict(mod="QPSK", samples_per_symbol=32, centre=0.45, level_db=20.0, start=60 * row, on=30 * row),
    ], 300.0)


def numpy_detections(iq, threshold_db=6.0, dc_guard=1):
    """detect_iq's detections from the numpy references alone (iq: flat interleaved int16): iq_spectrum_ref's spectrogram,
    iq_components_ref's threshold rule and components, and the host half of find_detections; as dicts with detect_iq's keys"""
    import iq_components_ref as C
    import iq_spectrum_ref as S
    w = F.design_window(E2E_NFFT)
    P = S.spectrogram(np.asarray(iq).reshape(-1), "ci16", E2E_NFFT, E2E_NFFT // 2, E2E_AVG, w, F.window_scale(w))[0].astype(np.float32)
    thresh = C.detection_threshold(P, threshold_db, dc_guard, "flat")
    _, records, count = C.components(P, thresh, 2, 3)
    found = F.detections_from_components(P, thresh, records.view(_cabi.IQ_COMPONENT), count, avg=E2E_AVG)
    return [d._asdict() for d in found]


def e2e_must_find(truth, min_rows=3):
    """the truth dwells the end-to-end conditions speak of: wholly inside the capture and at least min_rows spectrogram rows long"""
    row = E2E_NFFT // 2 * E2E_AVG
    return [t for t in range(len(truth)) if truth["whole"][t] and truth["stop_pair"][t] - truth["first_pair"][t] >= min_rows * row]
