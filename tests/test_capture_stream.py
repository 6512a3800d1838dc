"""capture._StreamCore, the bookkeeping of VTCNN2.detect_stream, driven without a GPU: the class does no arithmetic, it calls
injected functions, and here they are the numpy restatements the kernels are held to -- a plain numpy power spectrogram,
tests/iq_cfar_ref.py, tests/iq_components_ref.py -- and a classifier stub that returns a checksum of the pairs it is handed, so
that the pairs a record is cut from are part of every comparison.  The bar is the stream's own: the records of all push() calls
and close() together equal the one-shot run on the concatenated capture, for every chunking, and none appears twice.

The seam tests use a second set of stubs: the "capture" holds its own pair indices, the "spectrogram" looks the rows up in a
hand-drawn ratio and the "ratio" is the identity, so a component's rows can be put exactly where a seam hurts.

One documented difference to detect_iq: a stream that ends before its first row returns [], where the one-shot call raises."""
import types
import zlib

import numpy as np
import pytest

import iq_cfar_ref as K
import iq_components_ref as C
from modulationdetectioncnn_amd import capture

NFFT, AVG = 64, 2
HOP, ROW = NFFT // 2, AVG * (NFFT // 2)      # a row's stride in pairs; a row reads ROW + HOP pairs
CFAR = (3, 8, 1, 2)                          # train_rows, train_bins, guard_rows, guard_bins; the lower median
REACH_ROWS, REACH_BINS, MIN_ROWS, MIN_BINS = 2, 3, 3, 3
THRESH = K.cfar_threshold(NFFT, 6.0, 1)
WINDOW = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(NFFT) / NFFT)
FIELDS = ("first_row", "stop_row", "first_bin", "stop_bin", "cells", "centre", "bandwidth", "peak_db", "snr_db", "first_pair", "stop_pair")


# ---- the injected functions ---------------------------------------------------------------------------------------------------------
def cat(a, b):
    return b.copy() if a is None else np.concatenate((a, b))


def spectrogram(pairs):
    """float32 (rows, NFFT): every row the mean of its AVG Hann-windowed segments' powers, computed row by row"""
    z = pairs[0::2].astype(np.float64) + 1j * pairs[1::2].astype(np.float64)
    rows = 0 if z.size < NFFT else ((z.size - NFFT) // HOP + 1) // AVG
    out = np.empty((rows, NFFT), np.float32)
    for r in range(rows):
        seg = np.stack([z[(r * AVG + s) * HOP:(r * AVG + s) * HOP + NFFT] * WINDOW for s in range(AVG)])
        out[r] = (np.abs(np.fft.fft(seg, axis=1)) ** 2).mean(axis=0) / (32768.0 * WINDOW.sum()) ** 2
    return out


def ratio(spec):
    return K.cfar(spec, *CFAR, 500)[1]


def components(r):
    return C.components(r, THRESH, REACH_ROWS, REACH_BINS)[1]


def classify(r, pairs, records):
    """C.find_detections' tuples as dicts, plus `pairs_crc`: the checksum of exactly the pairs [first_pair, stop_pair) handed in"""
    out = []
    for d in C.find_detections(r, THRESH, records, len(records), 1, 1, None, AVG):
        rec = dict(zip(FIELDS, d))
        assert 0 <= rec["first_pair"] < rec["stop_pair"] <= pairs.size // 2
        rec["pairs_crc"] = zlib.crc32(np.ascontiguousarray(pairs[2 * rec["first_pair"]:2 * rec["stop_pair"]]).tobytes())
        out.append(rec)
    return out


def make_core(max_rows=4096, fns=(spectrogram, ratio, components, classify), train_rows=CFAR[0], min_rows=MIN_ROWS):
    return capture._StreamCore(NFFT, AVG, train_rows, REACH_ROWS, min_rows, MIN_BINS, max_rows, *fns, cat)


def one_shot(iq, fns=(spectrogram, ratio, components, classify), min_rows=MIN_ROWS):
    """detect_iq(floor="cfar", batched=True) in the same functions: the whole capture at once"""
    spec_fn, ratio_fn, comp_fn, classify_fn = fns
    r = ratio_fn(spec_fn(iq))
    recs = comp_fn(r)
    big = (recs["row_stop"] - recs["row_first"] >= min_rows) & (recs["bin_stop"] - recs["bin_first"] >= MIN_BINS)
    return sorted(classify_fn(r, iq, recs[big]), key=key)


def key(rec):
    return (rec["first_pair"], rec["centre"])


def stream(iq, sizes, core, watch=None):
    """push iq in chunks of the listed sizes (pairs; the list is repeated until the capture is used up), then close"""
    out, at, i = [], 0, 0
    while at < iq.size // 2:
        n = min(sizes[i % len(sizes)], iq.size // 2 - at)
        got = core.push(iq[2 * at:2 * (at + n)], n)
        assert got == sorted(got, key=key)
        out += got
        at, i = at + n, i + 1
        assert core.pairs_seen == at and core.pairs_held <= core.pairs_bound and core.F <= core.S
        if watch is not None:
            watch(core)
    out += core.close()
    assert core.pairs_held == 0
    return out


def without_cut(records):
    return sorted(({k: v for k, v in r.items() if k != "cut"} for r in records), key=key)


# ---- the capture: two bursts, a hopper's two dwells, two emitters that share bins at different times, over noise ---------------------
PAIRS = 63 * ROW + HOP + 17      # 63 rows and a rest
# (first pair, stop pair, centre in cycles per sample): every emitter is four tones a bin apart, about six bins wide
EMITTERS = ((5 * ROW, 14 * ROW, -0.30), (30 * ROW + 9, 41 * ROW, -0.30),                 # the same bins, at different times
            (8 * ROW, 20 * ROW + 31, 0.12), (44 * ROW, 58 * ROW, 0.31),                  # two bursts
            (22 * ROW, 30 * ROW, -0.10), (30 * ROW, 38 * ROW, 0.40))                     # a hopper's two dwells, back to back


@pytest.fixture(scope="module")
def scene():
    rng = np.random.default_rng(2016)
    n = np.arange(PAIRS)
    z = 40.0 * (rng.standard_normal(PAIRS) + 1j * rng.standard_normal(PAIRS))
    for a, b, fc in EMITTERS:
        for k in range(4):
            z[a:b] += 60.0 * np.exp(2j * np.pi * ((fc + k / NFFT) * n[a:b] + rng.uniform()))
    iq = np.rint(np.stack([z.real, z.imag], axis=1)).astype(np.int16).reshape(-1)
    whole = one_shot(iq)
    return iq, whole


def test_scene_is_not_trivial(scene):
    _, whole = scene
    assert len(whole) >= 6
    for a, b, fc in EMITTERS:      # every emitter is found about where it was put
        assert any(abs(r["centre"] - (fc + 1.5 / NFFT)) < 2.0 / NFFT and abs(r["first_pair"] - a) <= 4 * ROW and abs(r["stop_pair"] - b) <= 4 * ROW
                   for r in whole), (a, b, fc)


def random_sizes():
    rng = np.random.default_rng(7)
    sizes = rng.integers(0, 5 * ROW, 200)
    sizes[rng.integers(0, 200, 40)] = 0
    return [int(s) for s in sizes]


CHUNKINGS = {"row-1": [ROW - 1], "row": [ROW], "row+1": [ROW + 1], "prime": [97], "larger": [PAIRS + 1000], "one pair": [1, ROW + HOP],
             "random": random_sizes()}


@pytest.mark.parametrize("name", list(CHUNKINGS))
def test_stream_equals_one_shot_and_emits_once(scene, name):
    iq, whole = scene
    got = stream(iq, CHUNKINGS[name], make_core())
    assert not any(r["cut"] for r in got)
    assert len({(r["first_row"], r["stop_row"], r["first_bin"], r["stop_bin"]) for r in got}) == len(got)      # no record twice
    assert without_cut(got) == whole


def test_retention_follows_the_open_detections(scene):
    """pairs_held falls back once the detections have closed: at the end of a quiet stretch only the rows that still wait for
    their CFAR window, and the rest of a row, are held"""
    iq, _ = scene
    core, held = make_core(), []
    stream(iq, [ROW], core, watch=lambda c: held.append((c.pairs_seen, c.pairs_held, c.F, c.t0)))
    assert all(t0 <= F for _, _, F, t0 in held)
    assert min(h for _, h, _, _ in held[10:]) <= (CFAR[0] + REACH_ROWS + 3) * ROW + HOP
    assert max(h for _, h, _, _ in held) < PAIRS // 2      # never most of the capture


# ---- seams: hand-drawn ratios ---------------------------------------------------------------------------------------------------------
def drawn(boxes, rows):
    """(iq, fns) of a stream whose ratio IS the drawing: boxes of (first_row, stop_row, first_col, stop_col) in centred columns
    hold 8.0 + a little that depends on the cell, everything else 1.0; the capture holds its own pair indices"""
    R = np.ones((rows, NFFT), np.float32)
    for r0, r1, c0, c1 in boxes:
        for r in range(r0, r1):
            for c in range(c0, c1):
                R[r, c] = 8.0 + ((r * 7 + c * 3) % 11) / 16.0
    R = np.ascontiguousarray(np.roll(R, -(NFFT // 2), axis=1))      # natural positions
    pairs = rows * ROW + HOP
    iq = np.repeat(np.arange(pairs, dtype=np.int64), 2)

    def lookup(p):
        n, first = p.size // 2, int(p[0])
        assert first % ROW == 0      # the slice starts on a row boundary
        return R[first // ROW:first // ROW + (0 if n < NFFT else ((n - NFFT) // HOP + 1) // AVG)]

    def crc(r, p, records):
        out = classify(r, p, records)
        for rec in out:      # the pairs handed in are the capture's, from the window's first row on
            assert int(p[2 * rec["first_pair"]]) - rec["first_pair"] == int(p[0]) and int(p[0]) % ROW == 0
            rec["pairs_from"] = int(p[2 * rec["first_pair"]])
        return out

    return iq, (lookup, lambda s: s, components, crc)


def every_split(iq, fns, rows, whole, **kw):
    """one seam at every row (and, with train_rows, at every state of the finality lag), then row by row: always the one-shot records"""
    for train_rows in (0, 3):
        for s in range(rows + 2):
            got = stream(iq, [s * ROW + HOP, iq.size], make_core(fns=fns, train_rows=train_rows, **kw))
            assert without_cut(got) == whole, (train_rows, s)
            assert all(r["pairs_from"] == r["first_pair"] and not r["cut"] for r in got)
        assert without_cut(stream(iq, [ROW], make_core(fns=fns, train_rows=train_rows, **kw))) == whole


SEAM_CASES = {
    # with train_rows = 0 the seam after s rows makes rows [0, s) final: s = 12 is `reach_rows past the box's end`, 11 one row
    # past it, 9 one row before it; every_split runs them all
    "one box, rows 4..9": ([(4, 10, 20, 26)], 1),
    "two boxes joined only by the reach": ([(4, 8, 20, 26), (9, 13, 20, 26)], 1),            # row 8 is off: 7 -> 9 is two rows
    "two boxes one row too far apart": ([(4, 8, 20, 26), (10, 14, 20, 26)], 2),              # 7 -> 10 is three
    "thinner than min_rows at the seam, grows later": ([(4, 5, 20, 24), (6, 7, 22, 26), (8, 9, 20, 24), (10, 11, 22, 26)], 1),
    "stays thinner than min_rows": ([(4, 6, 20, 26)], 0),
    "joined sideways, late": ([(3, 12, 10, 14), (3, 12, 20, 24), (11, 12, 14, 20)], 1),      # two columns that only their last row joins
    "a short branch beside a long one": ([(2, 18, 30, 34), (2, 3, 34, 44), (2, 6, 44, 48)], 1),
}


@pytest.mark.parametrize("name", list(SEAM_CASES))
def test_seam_positions(name):
    boxes, expect = SEAM_CASES[name]
    rows = 20
    iq, fns = drawn(boxes, rows)
    whole = one_shot(iq, fns)
    assert len(whole) == expect
    every_split(iq, fns, rows, whole)


def test_named_seams_close_the_box_when_they_should():
    """the box's row_stop is 10 and reach_rows 2: it closes in the round in which 12 rows are final, not one earlier"""
    iq, fns = drawn([(4, 10, 20, 26)], 20)
    for train_rows in (0, 3):
        for rows_pushed, closed in ((9, False), (11, False), (12, True), (13, True)):
            core = make_core(fns=fns, train_rows=train_rows)
            got = core.push(iq[:2 * ((rows_pushed + train_rows) * ROW + HOP)], (rows_pushed + train_rows) * ROW + HOP)
            assert core.F == rows_pushed and (len(got) == 1) == closed
            assert core.t0 == (rows_pushed if closed else 4)      # held from the open box's first row on, else from the final rows' end
            assert len(got + core.close()) == 1


# ---- the ends -------------------------------------------------------------------------------------------------------------------------
def test_close_on_an_empty_or_short_stream_returns_nothing():
    assert make_core().close() == []
    core = make_core()
    assert core.push(np.zeros(2 * (ROW + HOP - 1), np.int16), ROW + HOP - 1) == []      # one pair short of the first row
    assert core.S == 0 and core.pairs_held == ROW + HOP - 1
    assert core.close() == [] and core.close() == []


# ---- the forced cut ---------------------------------------------------------------------------------------------------------------------
def test_forced_cut_tiles_a_continuous_emitter():
    rows, M = 45, 8
    tone, early, across = (0, rows, 10, 15), (2, 5, 40, 44), (13, 19, 40, 44)      # `across` lies over the cut at row 16
    iq, fns = drawn([tone, early, across], rows)
    whole = one_shot(iq, fns)
    assert [(r["first_row"], r["stop_row"]) for r in whole] == [(0, rows), (2, 5), (13, 19)]
    reference = None
    for sizes in ([ROW], [ROW - 1], [97], [5 * ROW + 3], [iq.size]):
        for train_rows in (0, 3):
            core = make_core(max_rows=M, fns=fns, train_rows=train_rows)
            assert core.pairs_bound == (M + train_rows + 1) * ROW + HOP - 1
            got = sorted(stream(iq, sizes, core), key=key)
            pieces = [r for r in got if r["first_bin"] == 10]
            assert [(r["first_row"], r["stop_row"]) for r in pieces] == [(a, min(a + M, rows)) for a in range(0, rows, M)]      # no gap, no overlap
            assert [r["cut"] for r in pieces] == [True] * (len(pieces) - 1) + [False]
            others = [(r["first_row"], r["stop_row"], r["cut"]) for r in got if r["first_bin"] == 40]
            assert others == [(2, 5, False), (13, 16, True), (16, 19, False)]
            assert all(r["stop_pair"] - r["first_pair"] <= core.pairs_bound and r["pairs_from"] == r["first_pair"] for r in got)
            if reference is None:
                reference = got
            assert got == reference      # the cuts depend on the rows, not on the chunks


# ---- arguments --------------------------------------------------------------------------------------------------------------------------
MODEL = types.SimpleNamespace(device_index=0)


def test_argument_errors():
    with pytest.raises(ValueError, match="whole capture"):
        capture.detect_stream(MODEL, "ci16", floor="flat")
    with pytest.raises(ValueError, match="balance_stats"):
        capture.detect_stream(MODEL, "ci16", balance=True)
    with pytest.raises(ValueError, match="max_rows"):
        capture.detect_stream(MODEL, "ci16", max_rows=0)
    with pytest.raises(ValueError):
        capture.detect_stream(MODEL, "cf32")
    s = capture.detect_stream(MODEL, "ci16", nfft=NFFT, avg=AVG)
    with pytest.raises(ValueError, match="odd"):
        s.push(np.zeros(7, np.int16))
    assert s.pairs_seen == 0 and s.pairs_held == 0 and s.rows_final == 0
    assert s.close() == []
    with capture.detect_stream(MODEL, "ci16") as t:      # leaving the block closes the stream
        pass
    for closed in (s, t):
        assert closed.close() == []
        with pytest.raises(ValueError, match="after close"):
            closed.push(np.zeros(8, np.int16))


def test_detect_stream_is_bound_to_the_model():
    from modulationdetectioncnn_amd import VTCNN2
    assert VTCNN2.detect_stream is capture.detect_stream
