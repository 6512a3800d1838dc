"""The end-to-end capture of tests/test_iq_cfar_gpu.py: one scene of bursts and a hopper rendered twice and concatenated, the
second render with the noise AND every emitter 10 dB up -- a receiver's gain step in the middle of the capture.  Built on the host
only (frontend.synth_scene); the render is frontend.synth_capture's."""
import numpy as np

from modulationdetectioncnn_amd import frontend as F

MODS = ("QPSK", "BPSK", "GFSK")
SEED = 2016
NFFT, AVG = 256, 8
ROW = NFFT // 2 * AVG              # capture pairs per spectrogram row
HALF_ROWS = 128
HALF_PAIRS = HALF_ROWS * ROW       # 2^17 pairs per render, 2^18 in all
NOISE_RMS, STEP_DB = 100.0, 10.0

_recipe = []


def recipe():
    if not _recipe:
        _recipe.append(F.synth_recipe(mods=MODS, snrs_db=(10,), sps=8, span=8))
    return _recipe[0]


def scenes():
    """(quiet, loud): the same emitters, 20 dB above the noise inside their bands, on noise of rms 100 and of rms 100 * 10^(10/20)"""
    emitters = [
        dict(mod="QPSK", samples_per_symbol=32, centre=-0.40, level_db=20.0, start=10 * ROW, on=20 * ROW, period=45 * ROW),
        dict(mod="BPSK", samples_per_symbol=32, centre=-0.10, level_db=20.0, start=30 * ROW, on=25 * ROW, period=60 * ROW),
        dict(mod="GFSK", samples_per_symbol=32, centre=[0.10, 0.20, 0.30, 0.40], level_db=20.0, start=5 * ROW, on=12 * ROW, period=20 * ROW),
    ]
    return tuple(F.synth_scene(recipe(), emitters, NOISE_RMS * 10.0 ** (db / 20.0)) for db in (0.0, STEP_DB))


def truth():
    """scene_truth of both renders as one array, the second render's pairs moved behind the first's"""
    quiet, loud = scenes()
    a, b = F.scene_truth(quiet, HALF_PAIRS, SEED), F.scene_truth(loud, HALF_PAIRS, SEED)
    b = b.copy()
    b["first_pair"] += HALF_PAIRS
    b["stop_pair"] += HALF_PAIRS
    return np.concatenate([a, b])


def must_find(truth, train_rows=8, min_rows=3):
    """the truth bursts the conditions speak of: whole, at least min_rows rows long, and at least train_rows rows from the seam"""
    seam, keep = HALF_PAIRS, []
    for t in range(len(truth)):
        a, z = int(truth["first_pair"][t]), int(truth["stop_pair"][t])
        clear = z <= seam - train_rows * ROW or a >= seam + train_rows * ROW
        if truth["whole"][t] and z - a >= min_rows * ROW and clear:
            keep.append(t)
    return keep
