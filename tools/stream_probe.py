#!/usr/bin/env python3
"""What VTCNN2.detect_stream costs next to VTCNN2.detect_iq(floor="cfar", batched=True) on the same capture, and what it holds.

All in this one process, warm, host clock around the whole run plus a device synchronise, median of `rounds` rounds (spread =
(max - min) / median):

  0. Self-check: the stream's records at every chunk size are detect_iq's -- boxes, plans, labels and window counts --, or the probe
     stops.
  1. detect_iq(floor="cfar", batched=True) on a synthetic "ci16" capture of 2^24 pairs on the device (bursts and a hopper,
     frontend.synth_capture; nfft 1024, avg 8: 4,095 rows of 4,096 pairs).
  2. detect_stream over the same capture in chunks of 2^18, 2^20 and 2^22 pairs (views of the device tensor: no transfer is
     timed): time, the ratio to (1), the peak of pairs_held, the mean number of new final rows per push and the mean retained
     tail (final rows still held after a push, which the next push labels again).
  3. Beside the ratio, the share the design predicts for the two kernels that see rows twice: a push of n rows runs the CFAR over n
     + 2 train_rows rows and the labelling over the n new final rows plus the retained tail, so (2 train_rows + tail) / n rows are
     recomputed.  What the design does not predict from rows is the fixed cost per push, which is what the measured ratio
     shows (about 3 ms per push): the launches (spectrogram, CFAR, three of the labelling, the joins) and the
     one read-back of the component count, and per push with a closed box detect_iq's batched extraction and forward on that
     push's boxes alone, with its filter designs on the host.

The scene has no emitter that never pauses: such a one keeps every row retained until max_rows cuts it, and the
labelling then runs over max_rows rows on every push; --continuous adds one, to see that case.

Needs the GPU; prints a table and one JSON line.

    python tools/stream_probe.py [--rounds 5] [--log2-pairs 24] [--continuous] [--max-rows 4096] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NFFT, AVG, ROW = 1024, 8, 4096
LOG2_CHUNKS = (18, 20, 22)
FIELDS = ("first_row", "stop_row", "first_bin", "stop_bin", "cells", "centre", "first_pair", "stop_pair", "shift", "interpolate", "decimate", "windows", "label")


def spread(times):
    return (max(times) - min(times)) / float(np.median(times))


def capture(pairs, F, continuous):
    recipe = F.synth_recipe(mods=("QPSK", "BPSK", "GFSK", "8PSK"), snrs_db=(10,), sps=8, span=8)
    emitters = [dict(mod="BPSK", samples_per_symbol=64, centre=-0.15, level_db=20.0, start=10 * ROW, on=20 * ROW, period=40 * ROW),
                dict(mod="GFSK", samples_per_symbol=64, centre=[0.05, 0.15, 0.25, 0.35], level_db=20.0, start=4 * ROW, on=12 * ROW, period=16 * ROW),
                dict(mod="8PSK", samples_per_symbol=64, centre=0.45, level_db=20.0, start=8 * ROW, on=24 * ROW, period=64 * ROW)]
    if continuous:
        emitters.insert(0, dict(mod="QPSK", samples_per_symbol=64, centre=-0.35, level_db=20.0))
    return F.synth_capture(pairs, F.synth_scene(recipe, emitters, 300.0), seed=2016), len(recipe.mods)


def run_stream(model, iq, chunk, max_rows, stats=None):
    out = []
    s = model.detect_stream("ci16", max_rows=max_rows)
    for at in range(0, iq.shape[0], 2 * chunk):
        before = s.rows_final
        out += s.push(iq[at:at + 2 * chunk])
        if stats is not None:
            stats.append((s.pairs_held, s.rows_final - before, s.rows_final - s._core.t0))
    return out + s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--log2-pairs", type=int, default=24)
    ap.add_argument("--continuous", action="store_true", help="add an emitter that never pauses (the forced cut's case)")
    ap.add_argument("--max-rows", type=int, default=4096)
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    a = ap.parse_args()
    import torch
    from modulationdetectioncnn_amd import VTCNN2, frontend as F
    pairs = 1 << a.log2_pairs
    iq, classes = capture(pairs, F, a.continuous)
    model = VTCNN2.synthetic("vtcnn2", classes=classes)
    train_rows = F.CFAR_DEFAULTS["train_rows"]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, got

    def one_shot():
        return model.detect_iq(iq, "ci16", floor="cfar", batched=True)

    _, want = timed(one_shot)      # warm
    times = [timed(one_shot)[0] for _ in range(a.rounds)]
    whole = dict(ms=float(np.median(times)) * 1e3, spread=spread(times), detections=len(want))
    rows = F.spectrogram_rows(pairs, NFFT, NFFT // 2, AVG)
    print(f"detect_iq(floor='cfar', batched=True) at 2^{a.log2_pairs} pairs ({rows} rows): {whole['ms']:.1f} ms ({whole['spread']:.2f}), "
          f"{len(want)} detections")
    want_key = sorted(tuple(r[k] for k in FIELDS) for r in want)
    chunks = []
    print(f"{'chunk':>8s} {'pushes':>7s} {'ms':>9s} {'spread':>7s} {'ratio':>6s} {'peak held':>10s} {'rows/push':>10s} {'tail rows':>9s} {'predicted':>10s} {'cut':>4s}")
    for lg in LOG2_CHUNKS:
        chunk, stats = 1 << lg, []
        _, got = timed(lambda: run_stream(model, iq, chunk, a.max_rows, stats))      # warm, and the statistics
        cuts = sum(r["cut"] for r in got)
        if not cuts and sorted(tuple(r[k] for k in FIELDS) for r in got) != want_key:
            sys.exit(f"self-check failed: the stream's records at chunks of 2^{lg} pairs are not detect_iq's")
        times = [timed(lambda: run_stream(model, iq, chunk, a.max_rows))[0] for _ in range(a.rounds)]
        ms = float(np.median(times)) * 1e3
        n = float(np.mean([s[1] for s in stats]))
        tail = float(np.mean([s[2] for s in stats]))
        predicted = (2 * train_rows + tail) / max(n, 1.0)
        chunks.append(dict(log2_chunk=lg, pushes=len(stats), ms=ms, spread=spread(times), ratio=ms / whole["ms"], peak_pairs_held=max(s[0] for s in stats),
                           rows_per_push=n, tail_rows_after_push=tail, predicted_recomputed_share=predicted, detections=len(got), cut=int(cuts)))
        print(f"{'2^' + str(lg):>8s} {len(stats):7d} {ms:9.1f} {spread(times):7.2f} {ms / whole['ms']:6.2f} {max(s[0] for s in stats):10d} {n:10.1f} {tail:9.1f} "
              f"{predicted:10.3f} {cuts:4d}")
    model._release()
    rec = dict(probe="stream", device=torch.cuda.get_device_name(0), log2_pairs=a.log2_pairs, rows=int(rows), continuous=bool(a.continuous),
               max_rows=a.max_rows, rounds=a.rounds, detect_iq=whole, detect_stream=chunks)
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
