#!/usr/bin/env python3
"""Throughput of mdc_iq_resample (frequency shift + low-pass + resampling by L/D, csrc/iq_resample.hip) on the device, next to
mdc_iq_ddc on the same data as the yardstick.

For CU8 and CI16 at (L, D) in {(1, 12), (5, 6), (25, 32), (8, 1)} with frontend.design_resampler's taps on 2^26 input pairs:
input pairs/s and GB/s (the bytes the algorithm needs: pair_bytes per input pair read once + 4 bytes per output pair written),
the HBM bound those bytes set at the measured copy rate of the MI355X (6.29 TB/s) and the packed-dot-product bound
(2 * ceil(B / 2) lane-operations per OUTPUT pair, B = ceil(T / L) the longest branch, on 256 CUs x 4 SIMDs x 32 lanes/clk at
2.4 GHz).  In the same run mdc_iq_ddc at (D, T) = (12, 96): the (1, 12) case does the same arithmetic on the same taps, so their
ratio is what the per-lane tap reads and the odd-start operand assembly of the resampler's filter cost.

Timing: device events around `reps` back-to-back launches after a warm-up, the median of `rounds` such windows, the cases
alternating within every round.  Needs the GPU; prints a table and one JSON line.

    python tools/resample_probe.py [--log2-pairs 26] [--rounds 5] [--reps 10] [--out FILE] [--lib PATH]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_COPY_BYTES_PER_S = 6.29e12
VALU_LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9
SHAPES = [(1, 12), (5, 6), (25, 32), (8, 1)]
DDC_SHAPE = (12, 96)


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
        raise SystemExit("resample_probe needs the GPU: a CPU run says nothing about speed")
    P = 1 << a.log2_pairs
    if a.lib:
        _cabi.LIB_PATHS["product"] = os.path.abspath(a.lib)      # before the first use: lib() loads once
    lib = _cabi.lib()
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(1)
    step = frontend.phase_step(-0.2)
    rows = []
    for fmt, name, dt, lo, hi in ((_cabi.IQ_CU8, "cu8", torch.uint8, 0, 256), (_cabi.IQ_CI16, "ci16", torch.int16, -32768, 32768)):
        iq = torch.randint(lo, hi, (2 * P,), dtype=dt, device="cuda", generator=g)
        pair_bytes = _cabi.IQ_PAIR_BYTES[fmt]
        cases = []
        for L, D in SHAPES:
            h = frontend.design_resampler(L, D)
            n_out = lib.mdc_iq_resample_out_count(P, h.size, L, D)
            out = torch.empty((n_out, 2), dtype=torch.int16, device="cuda")

            def run(L=L, D=D, h=h, n_out=n_out, out=out):
                _cabi.check(lib.mdc_iq_resample(iq.data_ptr(), fmt, P, 0, step, L, D, h.ctypes.data, h.size, out.data_ptr(), n_out, stream))

            cases.append(dict(kernel="mdc_iq_resample", L=L, D=D, T=int(h.size), n_out=n_out, run=run, out=out, times=[]))
        D, T = DDC_SHAPE
        h = frontend.design_lowpass(D, ntaps=T)
        n_out = lib.mdc_iq_ddc_out_count(P, T, D)
        out = torch.empty((n_out, 2), dtype=torch.int16, device="cuda")

        def ddc(D=D, T=T, h=h, n_out=n_out, out=out):
            _cabi.check(lib.mdc_iq_ddc(iq.data_ptr(), fmt, P, 0, step, D, h.ctypes.data, T, out.data_ptr(), n_out, stream))

        cases.append(dict(kernel="mdc_iq_ddc", L=1, D=D, T=T, n_out=n_out, run=ddc, out=out, times=[]))
        for c in cases:      # warm-up: code objects
            c["run"]()
            c["run"]()
        torch.cuda.synchronize()
        assert torch.equal(cases[0]["out"], cases[-1]["out"])      # (1, 12) and the DDC: the same bits
        for _ in range(a.rounds):
            for c in cases:
                c["times"].append(_time(c["run"], a.reps, torch))
        ddc_seconds = float(np.median(cases[-1]["times"]))
        for c in cases:
            t = float(np.median(c["times"]))
            nbytes = pair_bytes * P + 4 * c["n_out"]
            longest = -(-c["T"] // c["L"])
            dot_ops = 2 * ((longest + 1) // 2) * c["n_out"]
            rows.append(dict(kernel=c["kernel"], format=name, interpolate=c["L"], decimate=c["D"], ntaps=c["T"], pairs=P, n_out=c["n_out"],
                             seconds=t, seconds_min=float(min(c["times"])), pairs_per_s=P / t, gbytes_per_s=nbytes / t / 1e9,
                             hbm_bound_s=nbytes / HBM_COPY_BYTES_PER_S, dot2_bound_s=dot_ops / VALU_LANE_OPS_PER_S,
                             share_of_bound=max(nbytes / HBM_COPY_BYTES_PER_S, dot_ops / VALU_LANE_OPS_PER_S) / t,
                             seconds_over_ddc_12_96=t / ddc_seconds))
        del cases, iq, out
        torch.cuda.empty_cache()
    print(f"device: {torch.cuda.get_device_name(0)}; 2^{a.log2_pairs} input pairs; median of {a.rounds} windows of {a.reps} launches")
    print(f"{'kernel':16s} {'fmt':5s} {'L':>3s} {'D':>3s} {'T':>4s} {'ms':>8s} {'Gpairs/s':>9s} {'GB/s':>8s} {'HBM bound ms':>13s} {'dot2 bound ms':>14s} "
          f"{'of bound':>9s} {'x ddc(12,96)':>13s}")
    for r in rows:
        print(f"{r['kernel']:16s} {r['format']:5s} {r['interpolate']:3d} {r['decimate']:3d} {r['ntaps']:4d} {r['seconds'] * 1e3:8.3f} "
              f"{r['pairs_per_s'] / 1e9:9.2f} {r['gbytes_per_s']:8.1f} {r['hbm_bound_s'] * 1e3:13.3f} {r['dot2_bound_s'] * 1e3:14.3f} "
              f"{r['share_of_bound']:9.2f} {r['seconds_over_ddc_12_96']:13.2f}")
    rec = json.dumps({"tool": "resample_probe", "device": torch.cuda.get_device_name(0), "rows": rows})
    print(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(rec + "\n")


if __name__ == "__main__":
    main()
