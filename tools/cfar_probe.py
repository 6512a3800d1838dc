#!/usr/bin/env python3
"""What mdc_iq_spectrogram_cfar (csrc/iq_cfar.hip) costs, next to the floor path it stands beside and to a copy, and what share of a
whole VTCNN2.detect_iq(floor="cfar") call it is.

All in this one process, warm, device events around `reps` launches, median of `rounds` rounds (spread = (max - min) / median):

  0. Self-check: frontend.cfar_floor against tests/iq_cfar_ref.py on 37 x 128 at the defaults and 40 x 512 at the maxima, floor and
     ratio bit for bit, or the probe stops.
  1. The kernel (floor and ratio both) on 32,768 x 1,024 and 4,096 x 1,024 cells of chi-square noise, at the defaults (8, 32, 2, 8)
     and at the maxima (16, 128, 2, 8): time, cells/s, and the share of the copy's byte rate (4 bytes read + 8 written per cell over
     the time, against the copy's 8 bytes per cell over its time).
  2. frontend.detection_threshold(spec, floor="flat") on the same spectrograms: spectrum_quantiles(spec, 0.5) and the few torch
     launches behind it -- one number per bin.
  3. A device-to-device copy of the spectrogram.
  4. detect_iq(batched=True) on a synthetic capture of 2^24 pairs (bursts and a hopper, frontend.synth_capture), floor="cfar" and
     floor="flat": host clock around the call plus a device synchronise; and cfar_floor alone on that capture's spectrogram.  The
     floor's share of the call is the kernel's time over the call's.

Needs the GPU; prints tables and one JSON line.

    python tools/cfar_probe.py [--rounds 5] [--log2-pairs 24] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(32768, 1024), (4096, 1024)]
PARAMS = {"defaults": (8, 32, 2, 8), "maxima": (16, 128, 2, 8)}


def spread(times):
    return (max(times) - min(times)) / float(np.median(times))


def event_time(fn, reps, torch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def measure(fn, rounds, torch, budget=0.5):
    """(median, spread) of `rounds` rounds; reps sized from one warm call so that a round takes about `budget` seconds"""
    fn()
    torch.cuda.synchronize()
    once = event_time(fn, 1, torch)
    reps = int(min(50, max(1, budget / max(once, 1e-6))))
    times = [event_time(fn, reps, torch) for _ in range(rounds)]
    return float(np.median(times)), spread(times)


def noise(rows, nfft, torch):
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn((16, rows, nfft), generator=g, device="cuda", dtype=torch.float32)
    return (x * x).mean(dim=0).contiguous()      # chi-square, 16 degrees of freedom


def self_check(F, torch):
    import iq_cfar_ref as R
    rng = np.random.default_rng(1)
    for shape, params in (((37, 128), (8, 32, 2, 8, 500)), ((40, 512), (16, 128, 2, 8, 500))):
        P = (rng.chisquare(16, shape) / 16.0).astype(np.float32)
        want = R.cfar(P, *params)
        got = F.cfar_floor(torch.from_numpy(P).cuda(), *params[:4], rank=params[4] / 1000.0, return_ratio=True)
        for w, g, name in zip(want, got, ("floor", "ratio")):
            if not np.array_equal(w.view(np.uint32), g.cpu().numpy().view(np.uint32)):
                sys.exit(f"self-check failed: {name} differs from tests/iq_cfar_ref.py at {shape}, {params}")
    print("self-check: floor and ratio equal tests/iq_cfar_ref.py bit for bit (37 x 128 defaults, 40 x 512 maxima)")


def capture(pairs, F):
    row = 1024 // 2 * 8
    recipe = F.synth_recipe(mods=("QPSK", "BPSK", "GFSK", "8PSK"), snrs_db=(10,), sps=8, span=8)
    scene = F.synth_scene(recipe, [
        dict(mod="QPSK", samples_per_symbol=64, centre=-0.35, level_db=20.0),
        dict(mod="BPSK", samples_per_symbol=64, centre=-0.15, level_db=20.0, start=10 * row, on=20 * row, period=40 * row),
        dict(mod="GFSK", samples_per_symbol=64, centre=[0.05, 0.15, 0.25, 0.35], level_db=20.0, start=4 * row, on=12 * row, period=16 * row),
        dict(mod="8PSK", samples_per_symbol=64, centre=0.45, level_db=20.0, start=8 * row, on=24 * row, period=64 * row),
    ], 300.0)
    return F.synth_capture(pairs, scene, seed=2016), len(recipe.mods)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--log2-pairs", type=int, default=24)
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    a = ap.parse_args()
    import torch
    from modulationdetectioncnn_amd import VTCNN2, frontend as F
    self_check(F, torch)
    kernel, beside = [], []
    print("kernel (floor and ratio), the per-bin floor path beside it, and a copy (ms: median, spread)")
    for rows, nfft in SHAPES:
        spec = noise(rows, nfft, torch)
        cells = rows * nfft
        out = torch.empty_like(spec)
        t_copy, s_copy = measure(lambda: out.copy_(spec), a.rounds, torch)
        t_flat, s_flat = measure(lambda: F.detection_threshold(spec, 6.0, 1, "flat"), a.rounds, torch)
        beside.append(dict(rows=rows, nfft=nfft, copy_ms=t_copy * 1e3, copy_spread=s_copy, copy_bytes_per_s=8.0 * cells / t_copy,
                           flat_threshold_ms=t_flat * 1e3, flat_threshold_spread=s_flat))
        print(f"  {rows:6d} x {nfft}: copy {t_copy * 1e3:8.3f} ms ({s_copy:.2f}) = {8.0 * cells / t_copy / 1e12:.2f} TB/s;  detection_threshold('flat') "
              f"{t_flat * 1e3:8.3f} ms ({s_flat:.2f})")
        for name, p in PARAMS.items():
            t, s = measure(lambda: F.cfar_floor(spec, *p, rank=0.5, return_ratio=True), a.rounds, torch)
            share = (12.0 * cells / t) / (8.0 * cells / t_copy)
            kernel.append(dict(rows=rows, nfft=nfft, params=name, ms=t * 1e3, spread=s, cells_per_s=cells / t, share_of_copy_byte_rate=share))
            print(f"      cfar {name:8s} {p}: {t * 1e3:9.3f} ms ({s:.2f}) = {cells / t / 1e9:6.3f} Gcell/s, {100 * share:.3f} % of the copy's byte rate")
        del spec, out
    pairs = 1 << a.log2_pairs
    iq, classes = capture(pairs, F)
    model = VTCNN2.synthetic("vtcnn2", classes=classes)
    whole = {}
    for floor in ("cfar", "flat"):
        def call():
            t0 = time.perf_counter()
            recs = model.detect_iq(iq, "ci16", floor=floor, batched=True)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, len(recs)
        call()
        times = [call() for _ in range(a.rounds)]
        whole[floor] = dict(ms=float(np.median([t for t, _ in times])) * 1e3, spread=spread([t for t, _ in times]), detections=times[0][1])
    spec = F.spectrogram(iq, "ci16", nfft=1024, avg=8)
    t_floor, s_floor = measure(lambda: F.cfar_floor(spec, return_ratio=True), a.rounds, torch)
    share = t_floor * 1e3 / whole["cfar"]["ms"]
    model._release()
    print(f"detect_iq(batched=True) at 2^{a.log2_pairs} pairs ({spec.shape[0]} x 1024 cells): floor='cfar' {whole['cfar']['ms']:.1f} ms "
          f"({whole['cfar']['spread']:.2f}; {whole['cfar']['detections']} detections), floor='flat' {whole['flat']['ms']:.1f} ms ({whole['flat']['spread']:.2f}; "
          f"{whole['flat']['detections']} detections); cfar_floor alone {t_floor * 1e3:.3f} ms ({s_floor:.2f}) = {100 * share:.1f} % of the call, the rest "
          f"{whole['cfar']['ms'] - t_floor * 1e3:.1f} ms")
    rec = dict(probe="cfar", device=torch.cuda.get_device_name(0), kernel=kernel, beside=beside,
               detect_iq=dict(log2_pairs=a.log2_pairs, rows=int(spec.shape[0]), whole=whole, cfar_floor_ms=t_floor * 1e3, cfar_floor_spread=s_floor,
                              share_of_call=share))
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
