#!/usr/bin/env python3
"""Throughput of mdc_iq_balance_stats and mdc_iq_balance (csrc/iq_balance.hip) on the device, next to a device-to-device copy
in the same process as the yardstick.

Both kernels are HBM-bound streams: the statistics read pair_bytes per pair and write 40 bytes per block, the correction
reads pair_bytes and writes 4 bytes per pair.  Per format (CU8, CI8, CI16) on 2^24 pairs: the statistics at block_pairs
65536 (the default: 256 blocks, one work-group each) and 4096 (4096 blocks: the grid cap's 2048 work-groups, two steps each),
the correction, and a copy (Tensor.copy_ between two device buffers of the same dtype: hipMemcpyAsync, device to device) of
the bytes each case moves.  A copy of N bytes reads N and writes N; a kernel's byte rate is (bytes read + bytes written) / s,
and `of copy` is that rate over the copy's 2N / s.

Timing: device events around `reps` back-to-back launches after a warm-up, the median of `rounds` such windows, the cases
alternating within every round.  Needs the GPU; prints a table and one JSON line.

    python tools/balance_probe.py [--log2-pairs 24] [--rounds 5] [--reps 20] [--out FILE] [--lib PATH]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STATS_BLOCKS = (65536, 4096)
COEFFS = (328, -655, 17462, 720, 720, 15563)      # 1 dB / 5 degrees and a DC offset


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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    ap.add_argument("--lib", default=None, help="time this build of libmdc.so instead of the tree's (an A/B against a saved library)")
    a = ap.parse_args()
    import torch
    from modulationdetectioncnn_amd import _cabi
    if not torch.cuda.is_available():
        raise SystemExit("balance_probe needs the GPU: a CPU run says nothing about speed")
    P = 1 << a.log2_pairs
    if a.lib:
        _cabi.LIB_PATHS["product"] = os.path.abspath(a.lib)      # before the first use: lib() loads once
    lib = _cabi.lib()
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(1)
    rec = np.zeros((), _cabi.IQ_BALANCE_COEFFS)
    for name, v in zip(_cabi.IQ_BALANCE_COEFFS.names, COEFFS):
        rec[name] = v
    rows = []
    for fmt, name, dt, lo, hi in ((_cabi.IQ_CU8, "cu8", torch.uint8, 0, 256), (_cabi.IQ_CI8, "ci8", torch.int8, -128, 128),
                                  (_cabi.IQ_CI16, "ci16", torch.int16, -32768, 32768)):
        iq = torch.randint(lo, hi, (2 * P,), dtype=dt, device="cuda", generator=g)
        in_bytes = _cabi.IQ_PAIR_BYTES[fmt] * P
        out = torch.empty((P, 2), dtype=torch.int16, device="cuda")
        cases = []
        for B in STATS_BLOCKS:
            nb = lib.mdc_iq_balance_blocks(P, B)
            sums = torch.empty((nb, 5), dtype=torch.int64, device="cuda")

            def stats(B=B, nb=nb, sums=sums):
                _cabi.check(lib.mdc_iq_balance_stats(iq.data_ptr(), fmt, P, B, sums.data_ptr(), nb, stream))

            cases.append(dict(kernel="mdc_iq_balance_stats", block_pairs=B, bytes=in_bytes + 40 * nb, run=stats, keep=sums, times=[]))

        def balance():
            _cabi.check(lib.mdc_iq_balance(iq.data_ptr(), fmt, P, rec.ctypes.data, out.data_ptr(), stream))

        cases.append(dict(kernel="mdc_iq_balance", block_pairs=0, bytes=in_bytes + 4 * P, run=balance, keep=out, times=[]))
        for n in sorted({in_bytes // 2, (in_bytes + 4 * P) // 2}):      # copies moving 2N = the stats' / the correction's bytes
            src, dst = torch.empty((n,), dtype=torch.uint8, device="cuda"), torch.empty((n,), dtype=torch.uint8, device="cuda")

            def copy(src=src, dst=dst):
                dst.copy_(src, non_blocking=True)

            cases.append(dict(kernel="copy", block_pairs=0, bytes=2 * n, run=copy, keep=(src, dst), times=[]))
        for c in cases:      # warm-up: code objects
            c["run"]()
            c["run"]()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for c in cases:
                c["times"].append(_time(c["run"], a.reps, torch))
        copies = {c["bytes"]: c["bytes"] / float(np.median(c["times"])) for c in cases if c["kernel"] == "copy"}
        for c in cases:
            t = float(np.median(c["times"]))
            # the copy that moves the nearest byte count
            ref = copies[min(copies, key=lambda n: abs(n - c["bytes"]))]
            rows.append(dict(kernel=c["kernel"], format=name, block_pairs=c["block_pairs"], pairs=P, bytes=c["bytes"], seconds=t,
                             seconds_min=float(min(c["times"])), pairs_per_s=P / t if c["kernel"] != "copy" else None,
                             gbytes_per_s=c["bytes"] / t / 1e9, share_of_copy=c["bytes"] / t / ref))
        del cases, iq, out
        torch.cuda.empty_cache()
    print(f"device: {torch.cuda.get_device_name(0)}; 2^{a.log2_pairs} pairs; median of {a.rounds} windows of {a.reps} launches")
    print(f"{'kernel':22s} {'fmt':5s} {'block':>7s} {'MB moved':>9s} {'ms':>8s} {'Gpairs/s':>9s} {'GB/s':>8s} {'of copy':>8s}")
    for r in rows:
        gp = f"{r['pairs_per_s'] / 1e9:9.2f}" if r["pairs_per_s"] else f"{'-':>9s}"
        print(f"{r['kernel']:22s} {r['format']:5s} {r['block_pairs'] or '-':>7} {r['bytes'] / 1e6:9.1f} {r['seconds'] * 1e3:8.4f} {gp} "
              f"{r['gbytes_per_s']:8.1f} {r['share_of_copy']:8.2f}")
    out_rec = json.dumps({"tool": "balance_probe", "device": torch.cuda.get_device_name(0), "rows": rows})
    print(out_rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(out_rec + "\n")


if __name__ == "__main__":
    main()
