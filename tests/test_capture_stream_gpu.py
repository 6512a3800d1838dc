"""VTCNN2.detect_stream on the MI355X: the records of all push() calls and close() together are those of detect_iq(floor="cfar",
batched=True) on the whole capture -- key for key, floats and tensors compared with == / torch.equal, never a tolerance -- for
chunks that end inside a row, on a row and one pair after three rows, with and without refine, for device and numpy chunks, for
"cu8" and through a balance coefficients tuple; max_rows bounds what a stream holds against an emitter that never pauses; and
examples/classify_capture.py --stream prints the lines it prints without.

The scene is examples/score_detector.py's default at small rows (nfft 256, avg 2: a row is 256 pairs) and 2^16 pairs, its
continuous emitter switched on for a stretch in the middle, so that the stream's first retained row moves on both sides of it;
tests/iq_synth_capture_ref.py with the numpy restatements of spectrogram, CFAR and labelling gives 40-odd boxes for it, 30-odd of
them long enough for a window.  That the scene is not trivial is asserted before anything is compared."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from modulationdetectioncnn_amd import VTCNN2, Topology
from modulationdetectioncnn_amd import frontend as F

pytestmark = pytest.mark.gpu

NFFT, AVG, ROW, PAIRS, SEED = 256, 2, 256, 1 << 16, 2016
CFAR = (4, 16, 1, 2, 0.5)
MODS = ("QPSK", "BPSK", "GFSK", "8PSK")
KW = dict(nfft=NFFT, avg=AVG, cfar=CFAR)
REFINE = dict(line_nfft=128, line_avg=2, min_line_db=4.0)      # a box of 13 rows isolates to some 700 pairs: short line spectra, a low bar
CHUNKS = (4099, ROW, 3 * ROW + 1)


def kw(refine):
    return dict(KW, refine=True, **REFINE) if refine else KW


def emitters(continuous):
    always = {} if continuous else dict(start=96 * ROW, on=64 * ROW)
    return [dict(mod="QPSK", samples_per_symbol=32, centre=-0.35, level_db=20.0, **always),
            dict(mod="BPSK", samples_per_symbol=32, centre=-0.15, level_db=20.0, start=10 * ROW, on=20 * ROW, period=40 * ROW),
            dict(mod="GFSK", samples_per_symbol=32, centre=[0.05, 0.15, 0.25, 0.35], level_db=20.0, start=4 * ROW, on=12 * ROW, period=16 * ROW),
            dict(mod="8PSK", samples_per_symbol=32, centre=0.45, level_db=20.0, start=8 * ROW, on=24 * ROW),
            dict(mod="QPSK", samples_per_symbol=32, centre=0.45, level_db=20.0, start=60 * ROW, on=30 * ROW)]


def render(continuous):
    recipe = F.synth_recipe(mods=MODS, snrs_db=(0, 6, 12, 18))
    return F.synth_capture(PAIRS, F.synth_scene(recipe, emitters(continuous), 300.0), seed=SEED)


@pytest.fixture(scope="module")
def model():
    m = VTCNN2.synthetic(Topology.cnnpy(10, 10, 4))
    yield m
    m._release()


@pytest.fixture(scope="module")
def iq():
    return render(continuous=False)


@pytest.fixture(scope="module")
def whole(model, iq):
    """detect_iq's records of the whole capture, computed once: by refine"""
    return {refine: model.detect_iq(iq, "ci16", floor="cfar", batched=True, **kw(refine)) for refine in (False, True)}


def key(r):
    return (r["first_pair"], r["centre"])


def run(stream, capture, chunk):
    """(all records in detect_iq's order, the largest pairs_held after a push)"""
    out, held, flat = [], 0, capture.reshape(-1)
    for at in range(0, flat.shape[0], 2 * chunk):
        out += stream.push(flat[at:at + 2 * chunk])
        held = max(held, stream.pairs_held)
        assert stream.pairs_held <= stream.pairs_bound
    assert stream.pairs_seen == flat.shape[0] // 2
    out += stream.close()
    assert stream.pairs_held == 0
    return sorted(out, key=key), held


def same(got, want, numpy_out=False):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert [k for k in a if k != "cut"] == list(b) and a["cut"] is False
        for k in b:
            if isinstance(b[k], torch.Tensor):
                if numpy_out:
                    assert isinstance(a[k], np.ndarray) and a[k].dtype == b[k].cpu().numpy().dtype and np.array_equal(a[k], b[k].cpu().numpy()), k
                else:
                    assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
            else:
                assert type(a[k]) is type(b[k]) and a[k] == b[k], k


def test_the_scene_is_not_trivial(whole):
    for refine in (False, True):
        assert sum(r["windows"] >= 1 for r in whole[refine]) >= 6
    # refine had spectra to search and found lines: its five keys, and the plans they move, are compared in earnest
    assert sum(np.isfinite(r["symbol_line_db"]) for r in whole[True]) >= 6
    assert any(r["symbol_rate"] is not None for r in whole[True]) and any(r["carrier_order"] != 0 for r in whole[True])
    assert len({(r["interpolate"], r["decimate"]) for r in whole[False]}) >= 2


@pytest.mark.parametrize("refine", [False, True])
@pytest.mark.parametrize("chunk", CHUNKS)
def test_stream_equals_detect_iq(model, iq, whole, chunk, refine):
    got, held = run(model.detect_stream("ci16", **kw(refine)), iq, chunk)
    same(got, whole[refine])
    assert held < PAIRS // 2      # the stream let go of what had closed


@pytest.mark.parametrize("refine", [False, True])
@pytest.mark.parametrize("chunk", CHUNKS)
def test_numpy_chunks(model, iq, whole, chunk, refine):
    got, _ = run(model.detect_stream("ci16", **kw(refine)), iq.cpu().numpy(), chunk)
    same(got, whole[refine], numpy_out=True)


def test_cu8(model, iq):
    bytes_ = ((iq.to(torch.int32) >> 6) + 128).clamp(0, 255).to(torch.uint8)      # 20 dB emitters over about 5 LSB of noise
    want = model.detect_iq(bytes_, "cu8", floor="cfar", batched=True, **KW)
    assert sum(r["windows"] >= 1 for r in want) >= 6
    got, _ = run(model.detect_stream("cu8", **KW), bytes_, CHUNKS[0])
    same(got, want)


def test_balance_coefficients(model, iq):
    coeffs = F.BalanceCoeffs(37, -52, F.BALANCE_IDENTITY.m00, 0, F.BALANCE_IDENTITY.m00 // 16, F.BALANCE_IDENTITY.m11 - F.BALANCE_IDENTITY.m11 // 32)
    want = model.detect_iq(iq, "ci16", floor="cfar", batched=True, balance=coeffs, **KW)
    assert sum(r["windows"] >= 1 for r in want) >= 6 and all(r["image_rejection_db"] is None for r in want)
    got, _ = run(model.detect_stream("ci16", balance=coeffs, **KW), iq, CHUNKS[0])
    same(got, want)
    assert "image_rejection_db" in got[0]


def test_a_stream_of_one_push_and_arguments(model, iq, whole):
    with model.detect_stream("ci16", **KW) as s:
        got = s.push(iq)
        assert 0 < s.rows_final == F.spectrogram_rows(PAIRS, NFFT, NFFT // 2, AVG) - CFAR[0]
        got = sorted(got + s.close(), key=key)
    same(got, whole[False])
    with pytest.raises(ValueError):
        s.push(iq[:8])
    with pytest.raises(TypeError):
        model.detect_stream("ci16", **KW).push(iq.to(torch.int8))
    with pytest.raises(ValueError):
        model.detect_stream("ci16", floor="per-bin", **KW)
    with pytest.raises(ValueError):
        model.detect_stream("ci16", balance=True, **KW)


def test_forced_cut_bounds_a_continuous_emitter(model):
    """max_rows 8: pairs_bound = (8 + 4 + 1) * 256 + 127 = 3455 pairs, and the capture is 18 times that"""
    capture, M = render(continuous=True), 8
    s = model.detect_stream("ci16", max_rows=M, **KW)
    assert s.pairs_bound == (M + CFAR[0] + 1) * ROW + NFFT // 2 - 1 and PAIRS >= 16 * s.pairs_bound
    got, held = run(s, capture, CHUNKS[0])
    assert held <= s.pairs_bound
    assert all(r["stop_pair"] - r["first_pair"] <= s.pairs_bound and r["stop_row"] - r["first_row"] <= M for r in got)
    tone = sorted((r["first_row"], r["stop_row"], r["cut"]) for r in got if abs(r["centre"] + 0.35) < 0.01 and r["stop_row"] - r["first_row"] == M)
    assert len(tone) >= PAIRS // ROW // M - 2 and all(cut for _, _, cut in tone)
    assert all(b[0] == a[1] for a, b in zip(tone, tone[1:]))      # the pieces follow each other without gap or overlap
    assert any(not r["cut"] for r in got)
    again, _ = run(model.detect_stream("ci16", max_rows=M, **KW), capture, CHUNKS[2])      # the cuts depend on the rows, not on the chunks
    assert [(r["first_row"], r["stop_row"], r["first_bin"], r["stop_bin"], r["cut"], r["label"]) for r in again] == \
           [(r["first_row"], r["stop_row"], r["first_bin"], r["stop_bin"], r["cut"], r["label"]) for r in got]


def test_the_example_prints_the_same_lines(iq, tmp_path):
    """examples/classify_capture.py --detections --floor cfar on a file of the capture, with --stream and without: the same lines"""
    path = tmp_path / "capture.ci16"
    iq.cpu().numpy().astype("<i2").tofile(path)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = [sys.executable, os.path.join(root, "examples", "classify_capture.py"), str(path), "--format", "ci16", "--detections", "--batched", "--floor", "cfar",
            "--cfar", "4,16,1,2,0.5", "--nfft", str(NFFT), "--squelch", "-60"]

    def lines(extra):
        out = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        rows = [ln.split() for ln in out.stdout.splitlines()]
        return sorted((r for r in rows if len(r) == 9 and r[0].isdigit() and r[1].isdigit()), key=lambda r: (int(r[0]), float(r[2])))

    want = lines([])
    assert len(want) >= 6
    assert lines(["--stream", "4099"]) == want
    bad = subprocess.run(base[:-8] + ["--stream", "4099"], capture_output=True, text=True, timeout=120)      # without --floor cfar
    assert bad.returncode != 0 and "--floor cfar" in bad.stderr
