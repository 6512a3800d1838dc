#!/usr/bin/env python3
"""Throughput of mdc_iq_cf32_histogram and mdc_iq_cf32_quantize (csrc/iq_cf32.hip) on the device, next to a device-to-device
copy in the same process as the yardstick.

Both kernels are HBM-bound streams: the histogram reads 8 bytes per pair and adds at most 256 counts per work-group, the
quantiser reads 8 and writes 4 bytes per pair (its two counts are passed, as quantize_cf32(return_report=True) does).  Per size
(2^24 and 2^27 pairs) and input:
    gaussian   noise at a single scale: nearly every component in three to six adjacent exponent bins -- a real capture, and the
               histogram's worst case (the LDS counters it adds to are few)
    bits       uniform random 32-bit patterns: every exponent bin alike, 0.4 % non-finite values
both kernels and a copy (Tensor.copy_ between two device buffers: hipMemcpyAsync, device to device) of the bytes each moves.  A
copy of N bytes reads N and writes N; a kernel's byte rate is (bytes read + bytes written) / s, and `of copy` is that rate over
the copy's 2N / s.

Timing: device events around `reps` back-to-back launches after a warm-up, the median of `rounds` such windows, the cases
alternating within every round.  Needs the GPU; prints a table and one JSON line.

    python tools/cf32_probe.py [--log2-pairs 24 27] [--rounds 5] [--reps 10] [--out FILE] [--lib PATH]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    ap.add_argument("--log2-pairs", type=int, nargs="+", default=[24, 27])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    ap.add_argument("--lib", default=None, help="time this build of libmdc.so instead of the tree's (an A/B against a saved library)")
    a = ap.parse_args()
    import torch
    from modulationdetectioncnn_amd import _cabi
    if not torch.cuda.is_available():
        raise SystemExit("cf32_probe needs the GPU: a CPU run says nothing about speed")
    if a.lib:
        _cabi.LIB_PATHS["product"] = os.path.abspath(a.lib)      # before the first use: lib() loads once
    lib = _cabi.lib()
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(1)
    rows = []
    for lg in a.log2_pairs:
        P = 1 << lg
        out = torch.empty(2 * P, dtype=torch.int16, device="cuda")
        hist = torch.zeros(256, dtype=torch.int64, device="cuda")
        counts = torch.zeros(2, dtype=torch.int64, device="cuda")
        copies = {}
        for n in (4 * P, 6 * P):      # copies moving 2N = the histogram's 8 P / the quantiser's 12 P bytes
            copies[2 * n] = (torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda"))
        for name, gain in (("gaussian", 32768.0), ("bits", 1.0)):
            if name == "gaussian":
                iq = torch.randn(2 * P, dtype=torch.float32, device="cuda", generator=g) * 0.1
            else:
                iq = torch.randint(-2 ** 31, 2 ** 31, (2 * P,), dtype=torch.int32, device="cuda", generator=g).view(torch.float32)

            def histogram(iq=iq):
                _cabi.check(lib.mdc_iq_cf32_histogram(iq.data_ptr(), P, hist.data_ptr(), stream))

            def quantize(iq=iq, gain=gain):
                _cabi.check(lib.mdc_iq_cf32_quantize(iq.data_ptr(), P, gain, out.data_ptr(), counts.data_ptr(), stream))

            cases = [dict(kernel="mdc_iq_cf32_histogram", bytes=8 * P + 8 * 256, run=histogram, times=[]),
                     dict(kernel="mdc_iq_cf32_quantize", bytes=12 * P, run=quantize, times=[])]
            for nbytes, (src, dst) in copies.items():

                def copy(src=src, dst=dst):
                    dst.copy_(src, non_blocking=True)

                cases.append(dict(kernel="copy", bytes=nbytes, run=copy, times=[]))
            for c in cases:      # warm-up: code objects
                c["run"]()
                c["run"]()
            torch.cuda.synchronize()
            for _ in range(a.rounds):
                for c in cases:
                    c["times"].append(_time(c["run"], a.reps, torch))
            rate = {c["bytes"]: c["bytes"] / float(np.median(c["times"])) for c in cases if c["kernel"] == "copy"}
            for c in cases:
                t = float(np.median(c["times"]))
                ref = rate[min(rate, key=lambda n: abs(n - c["bytes"]))]      # the copy that moves the nearest byte count
                rows.append(dict(kernel=c["kernel"], input=name, log2_pairs=lg, pairs=P, bytes=c["bytes"], seconds=t,
                                 seconds_min=float(min(c["times"])), pairs_per_s=P / t if c["kernel"] != "copy" else None,
                                 gbytes_per_s=c["bytes"] / t / 1e9, share_of_copy=c["bytes"] / t / ref))
            del cases, iq
        del out, copies
        torch.cuda.empty_cache()
    print(f"device: {torch.cuda.get_device_name(0)}; median of {a.rounds} windows of {a.reps} launches")
    print(f"{'kernel':22s} {'input':9s} {'pairs':>6s} {'MB moved':>9s} {'ms':>8s} {'Gpairs/s':>9s} {'GB/s':>8s} {'of copy':>8s}")
    for r in rows:
        gp = f"{r['pairs_per_s'] / 1e9:9.2f}" if r["pairs_per_s"] else f"{'-':>9s}"
        print(f"{r['kernel']:22s} {r['input']:9s} {'2^%d' % r['log2_pairs']:>6s} {r['bytes'] / 1e6:9.1f} {r['seconds'] * 1e3:8.4f} {gp} "
              f"{r['gbytes_per_s']:8.1f} {r['share_of_copy']:8.2f}")
    out_rec = json.dumps({"tool": "cf32_probe", "device": torch.cuda.get_device_name(0), "rows": rows})
    print(out_rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(out_rec + "\n")


if __name__ == "__main__":
    main()
