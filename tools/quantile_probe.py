#!/usr/bin/env python3
"""Time of mdc_iq_spectrum_quantiles (per-bin order statistics of a spectrogram along time, csrc/iq_quantiles.hip) on the device,
next to torch.kthvalue as the yardstick.

For the ranks of q = (0.5, 0.98) on (rows, nfft) in {(16384, 1024), (65536, 256), (4096, 4096)} float32 spectrograms of
exponentially distributed values (what a noise spectrogram holds): milliseconds, the ratio to the yardstick, and the share of the
HBM floor -- rows * nfft * 4 bytes read once at the measured copy rate of the MI355X (6.29 TB/s); the kernel reads its tile
1 + 3 ceil(nranks / group) times, all but the first from L2 where the tile fits.  The yardstick, in the same process on the same
tensor: two torch.kthvalue(spec, rank + 1, dim=0) calls.  Both results are compared bit for bit before anything is timed.

Timing: device events around `reps` back-to-back launches after a warm-up, the median of `rounds` such windows, kernel and
yardstick alternating.  Needs the GPU; prints a table and one JSON line.

    python tools/quantile_probe.py [--rounds 5] [--reps 10] [--out profiles/quantile_probe.json] [--lib PATH] [--label TEXT]
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
SHAPES = [(16384, 1024), (65536, 256), (4096, 4096)]
QUANTILES = (0.5, 0.98)


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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    ap.add_argument("--lib", default=None, help="time this build of libmdc.so instead of the tree's (an A/B of tile widths: -DMDC_QUANTILE_TILE=N)")
    ap.add_argument("--label", default=None, help="a word for the record, e.g. the tile width of --lib")
    a = ap.parse_args()
    import torch
    from modulationdetectioncnn_amd import _cabi
    if not torch.cuda.is_available():
        raise SystemExit("quantile_probe needs the GPU: a CPU run says nothing about speed")
    if a.lib:
        _cabi.LIB_PATHS["product"] = os.path.abspath(a.lib)      # before the first use: lib() loads once
    L = _cabi.lib()
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(1)
    table = []
    for rows, nfft in SHAPES:
        spec = torch.empty((rows, nfft), dtype=torch.float32, device="cuda").exponential_(1.0, generator=g) * 1e-6
        ranks = np.array([math.floor(q * (rows - 1)) for q in QUANTILES], np.int64)
        out = torch.empty((ranks.size, nfft), dtype=torch.float32, device="cuda")

        def ours():
            _cabi.check(L.mdc_iq_spectrum_quantiles(spec.data_ptr(), rows, nfft, ranks.ctypes.data, ranks.size, out.data_ptr(), stream))

        def kth():
            return [torch.kthvalue(spec, int(r) + 1, dim=0).values for r in ranks]

        for fn in (ours, kth):      # warm-up: code objects, allocator
            fn()
            fn()
        torch.cuda.synchronize()
        if not torch.equal(out.view(torch.int32), torch.stack(kth()).view(torch.int32)):
            raise SystemExit(f"({rows}, {nfft}): the kernel and torch.kthvalue disagree")
        t_ours, t_kth = [], []
        for _ in range(a.rounds):
            t_ours.append(_time(ours, a.reps, torch))
            t_kth.append(_time(kth, max(1, a.reps // 5), torch))
        to, tk = float(np.median(t_ours)), float(np.median(t_kth))
        floor = rows * nfft * 4 / HBM_COPY_BYTES_PER_S
        table.append(dict(rows=rows, nfft=nfft, ranks=[int(r) for r in ranks], seconds=to, seconds_min=float(min(t_ours)), hbm_floor_s=floor,
                          share_of_hbm_floor=floor / to, kthvalue_seconds=tk, speedup_over_kthvalue=tk / to))
        del spec, out
        torch.cuda.empty_cache()
    print(f"device: {torch.cuda.get_device_name(0)}; q = {QUANTILES}; median of {a.rounds} windows of {a.reps} launches"
          + (f"; {a.label}" if a.label else ""))
    print(f"{'rows':>7s} {'nfft':>5s} {'ms':>8s} {'HBM floor ms':>13s} {'of floor':>9s} {'kthvalue ms':>12s} {'x kthvalue':>11s}")
    for r in table:
        print(f"{r['rows']:7d} {r['nfft']:5d} {r['seconds'] * 1e3:8.3f} {r['hbm_floor_s'] * 1e3:13.4f} {r['share_of_hbm_floor']:9.3f} "
              f"{r['kthvalue_seconds'] * 1e3:12.3f} {r['speedup_over_kthvalue']:11.1f}")
    rec = json.dumps({"tool": "quantile_probe", "device": torch.cuda.get_device_name(0), "label": a.label, "tile": _cabi.QUANTILES_TILE if not a.lib else None,
                      "rows": table})
    print(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(rec + "\n")


if __name__ == "__main__":
    main()
