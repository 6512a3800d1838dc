#!/usr/bin/env python3
"""Throughput of mdc_iq_spectrogram (windowed FFTs + averaged power, csrc/iq_spectrogram.hip) on the device.

For nfft in {256, 1024, 4096} x CU8, CI8 and CI16 at hop == nfft (every pair is transformed exactly once), avg = 16, Hann window,
on 2^26 input pairs: input pairs/s and GB/s (the bytes the algorithm needs: pair_bytes per input pair read once + 4 bytes per
output bin written), next to two roofs:
  HBM    those bytes at the measured copy rate of the MI355X (6.29 TB/s);
  VALU   5 log2(nfft) flop per pair -- the textbook count of a radix-2 complex FFT; window, conversion and |X|^2 come on top --
         against the f32 vector rate without packed math, 256 CUs x 4 SIMDs x 16 lanes/clk x 2 flop (FMA) at 2.4 GHz = 78.6 Tflop/s.
At hop == nfft a CU8 capture brings 2 bytes per pair against 40..60 flop: the VALU roof is the nearer one at every size here (and
the kernel's LDS traffic, one 8-byte read and write per pair and pass, nearer still: DESIGN.md).

Timing: device events around `reps` back-to-back launches after a warm-up, the median of `rounds` such windows, the cases
alternating within every round.  Needs the GPU; prints a table and one JSON line.

    python tools/spectrogram_probe.py [--log2-pairs 26] [--rounds 5] [--reps 10] [--out FILE] [--lib PATH]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_COPY_BYTES_PER_S = 6.29e12
VALU_F32_FLOP_PER_S = 256 * 4 * 16 * 2 * 2.4e9
NFFTS = [256, 1024, 4096]
AVG = 16


def _time(fn, reps, torch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-pairs", type=int, default=26)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    ap.add_argument("--lib", default=None, help="time this build of libmdc.so instead of the tree's (an A/B against a saved library)")
    a = ap.parse_args()
    import torch
    from modulationdetectioncnn_amd import _cabi, frontend
    if not torch.cuda.is_available():
        raise SystemExit("spectrogram_probe needs the GPU: a CPU run says nothing about speed")
    P = 1 << a.log2_pairs
    if a.lib:
        _cabi.LIB_PATHS["product"] = os.path.abspath(a.lib)      # before the first use: lib() loads once
    lib = _cabi.lib()
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(1)
    rows_out = []
    for fmt, name, dt, lo, hi in ((_cabi.IQ_CU8, "cu8", torch.uint8, 0, 256), (_cabi.IQ_CI8, "ci8", torch.int8, -128, 128),
                                  (_cabi.IQ_CI16, "ci16", torch.int16, -32768, 32768)):
        iq = torch.randint(lo, hi, (2 * P,), dtype=dt, device="cuda", generator=g)
        pair_bytes = _cabi.IQ_PAIR_BYTES[fmt]
        cases = []
        for nfft in NFFTS:
            w = frontend.design_window(nfft)
            wdev, scale = torch.from_numpy(w).cuda(), frontend.window_scale(w)
            rows = lib.mdc_iq_spectrogram_rows(P, nfft, nfft, AVG)
            out = torch.empty((rows, nfft), dtype=torch.float32, device="cuda")

            def run(nfft=nfft, wdev=wdev, scale=scale, rows=rows, out=out):
                _cabi.check(lib.mdc_iq_spectrogram(iq.data_ptr(), fmt, P, nfft, nfft, AVG, wdev.data_ptr(), scale, out.data_ptr(), rows, stream))

            cases.append(dict(nfft=nfft, rows=rows, run=run, out=out, wdev=wdev, times=[]))
        for c in cases:      # warm-up: code objects
            c["run"]()
            c["run"]()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for c in cases:
                c["times"].append(_time(c["run"], a.reps, torch))
        for c in cases:
            t = float(np.median(c["times"]))
            used = c["rows"] * AVG * c["nfft"]                     # pairs the rows cover (trailing segments are dropped)
            nbytes = pair_bytes * used + 4 * c["rows"] * c["nfft"]
            flop = 5.0 * math.log2(c["nfft"]) * used
            rows_out.append(dict(kernel="mdc_iq_spectrogram", format=name, nfft=c["nfft"], hop=c["nfft"], avg=AVG, pairs=used, rows=c["rows"],
                                 seconds=t, seconds_min=float(min(c["times"])), pairs_per_s=used / t, gbytes_per_s=nbytes / t / 1e9,
                                 hbm_bound_s=nbytes / HBM_COPY_BYTES_PER_S, valu_bound_s=flop / VALU_F32_FLOP_PER_S,
                                 share_of_bound=max(nbytes / HBM_COPY_BYTES_PER_S, flop / VALU_F32_FLOP_PER_S) / t))
        del cases, iq, out
        torch.cuda.empty_cache()
    print(f"device: {torch.cuda.get_device_name(0)}; 2^{a.log2_pairs} input pairs, hop == nfft, avg {AVG}; median of {a.rounds} windows of {a.reps} launches")
    print(f"{'fmt':5s} {'nfft':>5s} {'rows':>7s} {'ms':>8s} {'Gpairs/s':>9s} {'GB/s':>8s} {'HBM bound ms':>13s} {'VALU bound ms':>14s} {'of bound':>9s}")
    for r in rows_out:
        print(f"{r['format']:5s} {r['nfft']:5d} {r['rows']:7d} {r['seconds'] * 1e3:8.3f} {r['pairs_per_s'] / 1e9:9.2f} {r['gbytes_per_s']:8.1f} "
              f"{r['hbm_bound_s'] * 1e3:13.3f} {r['valu_bound_s'] * 1e3:14.3f} {r['share_of_bound']:9.2f}")
    rec = json.dumps({"tool": "spectrogram_probe", "device": torch.cuda.get_device_name(0), "rows": rows_out})
    print(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(rec + "\n")


if __name__ == "__main__":
    main()
