#!/usr/bin/env python3
"""Throughput of mdc_iq_channelizer (polyphase filter bank, csrc/iq_channelizer.hip) on the device.

For M in {16, 64, 256, 1024} channels, D = M / 2, frontend.design_channelizer's 8 M taps, on a ci16 capture of 2^24 input pairs:
input pairs/s, next to two roofs per input pair:
  HBM    4 bytes in + 4 M / D = 8 bytes out at the measured copy rate of the MI355X (6.29 TB/s);
  VALU   2 T / D = 32 integer multiply-adds (the prototype filter: T taps x re, im per step, one step per D pairs) and
         5 M log2(M) / D = 10 log2(M) flop (the textbook count of a radix-2 complex FFT per step), a multiply-add counted as two
         operations, against the f32 vector rate without packed math, 256 CUs x 4 SIMDs x 16 lanes/clk x 2 at 2.4 GHz = 78.6 Top/s.
For M = 16 and 64 also the route that existed before the channelizer, in the same process: M back-to-back frontend.ddc calls, one
per channel, each with shift -k / M, decimation D and frontend.design_lowpass(D)'s 8 D taps -- M passes over the capture.

Timing: device events around `reps` back-to-back launches after a warm-up, the median of `rounds` such windows, the cases
alternating within every round.  Needs the GPU; prints a table and one JSON line.

    python tools/channelizer_probe.py [--log2-pairs 24] [--rounds 5] [--reps 10] [--out FILE] [--lib PATH]
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
VALU_OP_PER_S = 256 * 4 * 16 * 2 * 2.4e9
CHANNELS = [16, 64, 256, 1024]
DDC_ROUTE = [16, 64]


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
    ap.add_argument("--log2-pairs", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    ap.add_argument("--lib", default=None, help="time this build of libmdc.so instead of the tree's (an A/B against a saved library)")
    a = ap.parse_args()
    import torch
    from modulationdetectioncnn_amd import _cabi, frontend
    if not torch.cuda.is_available():
        raise SystemExit("channelizer_probe needs the GPU: a CPU run says nothing about speed")
    P = 1 << a.log2_pairs
    if a.lib:
        _cabi.LIB_PATHS["product"] = os.path.abspath(a.lib)      # before the first use: lib() loads once
    lib = _cabi.lib()
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(1)
    iq = torch.randint(-32768, 32768, (2 * P,), dtype=torch.int16, device="cuda", generator=g)
    cases = []
    for M in CHANNELS:
        D = M // 2
        h, shift = frontend.design_channelizer(M)
        hdev = torch.from_numpy(h).cuda()
        n_out = lib.mdc_iq_channelizer_out_count(P, M, h.size, D)
        out = torch.empty((M, n_out, 2), dtype=torch.int16, device="cuda")

        def run(M=M, D=D, hdev=hdev, T=h.size, shift=shift, out=out, n_out=n_out):
            _cabi.check(lib.mdc_iq_channelizer(iq.data_ptr(), _cabi.IQ_CI16, P, 0, M, D, hdev.data_ptr(), T, shift, out.data_ptr(), n_out, stream))

        cases.append(dict(route="channelizer", M=M, D=D, T=int(h.size), run=run, reps=a.reps, times=[], keep=(out, hdev)))
    for M in DDC_ROUTE:
        D = M // 2
        taps = frontend.design_lowpass(D)

        def run_ddc(M=M, D=D, taps=taps):
            for k in range(M):
                frontend.ddc(iq, "ci16", shift=-k / M if 2 * k <= M else (M - k) / M, decimate=D, taps=taps)

        cases.append(dict(route="ddc x M", M=M, D=D, T=int(taps.size), run=run_ddc, reps=max(1, a.reps // 5), times=[]))
    for c in cases:      # warm-up: code objects, the allocator's blocks
        c["run"]()
        c["run"]()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for c in cases:
            c["times"].append(_time(c["run"], c["reps"], torch))
    rows = []
    for c in cases:
        t = float(np.median(c["times"]))
        M, D = c["M"], c["D"]
        row = dict(route=c["route"], channels=M, decimate=D, ntaps=c["T"], pairs=P, seconds=t, seconds_min=float(min(c["times"])), pairs_per_s=P / t)
        if c["route"] == "channelizer":
            nbytes = (4 + 4 * M / D) * P
            ops = (2 * 2 * c["T"] / D + 5 * M * math.log2(M) / D) * P
            row.update(hbm_bound_s=nbytes / HBM_COPY_BYTES_PER_S, valu_bound_s=ops / VALU_OP_PER_S,
                       share_of_bound=max(nbytes / HBM_COPY_BYTES_PER_S, ops / VALU_OP_PER_S) / t)
        rows.append(row)
    by = {(r["route"], r["channels"]): r for r in rows}
    for M in DDC_ROUTE:
        by["channelizer", M]["speedup_over_ddc_route"] = by["ddc x M", M]["seconds"] / by["channelizer", M]["seconds"]
    print(f"device: {torch.cuda.get_device_name(0)}; ci16, 2^{a.log2_pairs} input pairs, D = M / 2; median of {a.rounds} windows")
    print(f"{'route':12s} {'M':>5s} {'taps':>6s} {'ms':>9s} {'Gpairs/s':>9s} {'HBM bound ms':>13s} {'VALU bound ms':>14s} {'of bound':>9s} {'x ddc route':>12s}")
    for r in rows:
        if r["route"] == "channelizer":
            sp = f"{r['speedup_over_ddc_route']:12.2f}" if "speedup_over_ddc_route" in r else f"{'':12s}"
            print(f"{r['route']:12s} {r['channels']:5d} {r['ntaps']:6d} {r['seconds'] * 1e3:9.3f} {r['pairs_per_s'] / 1e9:9.2f} "
                  f"{r['hbm_bound_s'] * 1e3:13.3f} {r['valu_bound_s'] * 1e3:14.3f} {r['share_of_bound']:9.2f} {sp}")
        else:
            print(f"{r['route']:12s} {r['channels']:5d} {r['ntaps']:6d} {r['seconds'] * 1e3:9.3f} {r['pairs_per_s'] / 1e9:9.2f}")
    rec = json.dumps({"tool": "channelizer_probe", "device": torch.cuda.get_device_name(0), "rows": rows})
    print(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(rec + "\n")


if __name__ == "__main__":
    main()
