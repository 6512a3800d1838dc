#!/usr/bin/env python3
"""Cost of the signed 8- / 16-bit normalising kernels (mdc_iq_windows_norm, csrc/iq_formats.hip) against the unsigned-byte
kernel they were modelled on (mdc_iq_u8_windows_norm: the yardstick), on the MI355X, in ONE process, HIP-event medians:
frames + statistics over 2^20 windows at hops 128 and 16, for CU8 (old entry), CI8 and CI16, with the bytes each moves.

If all three are bandwidth-bound the traffic predicts CI16 <= (1024 + 512) / (1024 + 256) = 1.2 x the u8 time at hop 128 and
CI8 at parity; 10 % on top is allowed for run-to-run spread inside one process.  The record says whether each ratio is inside.

Writes profiles/iq_formats_timing.json (or --out).  Run it under `timeout`; it needs the GPU and has no fallback.
    timeout -k 10 300 python tools/time_iq_formats.py [--windows 1048576] [--reps 30] [--out profiles/iq_formats_timing.json] [--lib PATH]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from modulationdetectioncnn_amd import _cabi      # noqa: E402

HBM_PEAK = 8.0e12      # bytes/s, DESIGN.md's roof
SPREAD = 1.10          # allowance for run-to-run spread inside one process


def median_ms(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iq_formats_timing.json"))
    ap.add_argument("--lib", default=None, help="time this build of libmdc.so instead of the tree's (an A/B against a saved library)")
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be >= 20")
    if not torch.cuda.is_available():
        sys.exit("no ROCm device: nothing is measured without the GPU")
    n = a.windows
    if a.lib:
        _cabi.LIB_PATHS["product"] = os.path.abspath(a.lib)      # before the first use: lib() loads once
    L = _cabi.lib()
    stream = torch.cuda.current_stream().cuda_stream
    x = torch.empty((n, 2, 128), dtype=torch.float32, device="cuda")
    st32 = torch.empty((n, 4), dtype=torch.int32, device="cuda")
    st64 = torch.empty((n, 4), dtype=torch.int64, device="cuda")
    out = {"device": torch.cuda.get_device_name(0), "windows": n, "reps": a.reps, "spread_allowance": SPREAD,
           "method": "HIP events around one launch, median of reps after 5 warm-up launches; the yardstick is timed first and again last",
           "hops": {}}
    xp = x.data_ptr()
    for hop in (128, 16):
        pairs = hop * (n - 1) + 128
        u8 = torch.randint(0, 256, (2 * pairs,), dtype=torch.uint8, device="cuda")
        i8 = torch.randint(-128, 128, (2 * pairs,), dtype=torch.int8, device="cuda")
        i16 = torch.randint(-32768, 32768, (2 * pairs,), dtype=torch.int16, device="cuda")
        rec = {}

        def kernel(name, fn, bytes_in, bytes_stats):
            med, lo, hi = median_ms(fn, a.reps)
            moved = n * (bytes_in + 1024 + bytes_stats)      # distinct input bytes per window (hop pairs) + the frame + the record
            rec[name] = {"median_ms": med, "min_ms": lo, "max_ms": hi, "bytes_per_window": bytes_in + 1024 + bytes_stats, "bytes_moved": moved,
                         "TB_per_s": moved / (med * 1e-3) / 1e12, "fraction_of_hbm_peak": moved / (med * 1e-3) / HBM_PEAK}
            print(f"hop {hop}", name, rec[name], flush=True)

        def old():
            _cabi.check(L.mdc_iq_u8_windows_norm(u8.data_ptr(), n, hop, 7.8e-3, 1, xp, st32.data_ptr(), stream))

        kernel("u8 (mdc_iq_u8_windows_norm)", old, 2 * hop, 16)
        kernel("ci8", lambda: _cabi.check(L.mdc_iq_windows_norm(i8.data_ptr(), _cabi.IQ_CI8, n, hop, 7.8e-3, 1, xp, st64.data_ptr(), stream)), 2 * hop, 32)
        kernel("ci16", lambda: _cabi.check(L.mdc_iq_windows_norm(i16.data_ptr(), _cabi.IQ_CI16, n, hop, 7.8e-3, 1, xp, st64.data_ptr(), stream)), 4 * hop, 32)
        kernel("u8 (again)", old, 2 * hop, 16)
        yard = min(rec["u8 (mdc_iq_u8_windows_norm)"]["median_ms"], rec["u8 (again)"]["median_ms"])
        for name in ("ci8", "ci16"):
            predicted = (1024 + (4 if name == "ci16" else 2) * hop) / (1024 + 2 * hop)      # frames + input; the records (16 / 32 B) left out
            ratio = rec[name]["median_ms"] / yard
            rec[name + "_over_u8"] = {"ratio": ratio, "traffic_ratio": predicted, "allowed": predicted * SPREAD, "inside": ratio <= predicted * SPREAD}
            print(f"hop {hop}", name, "/ u8:", rec[name + "_over_u8"], flush=True)
        out["hops"][str(hop)] = rec
        del u8, i8, i16
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
