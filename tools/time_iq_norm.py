#!/usr/bin/env python3
"""Cost of the level-normalising front-end (mdc_iq_u8_windows_norm) on the MI355X, in ONE process, HIP-event medians:

  * mdc_iq_u8_windows (the plain conversion kernel: the yardstick) against the new kernel with frames + statistics, frames
    alone, and statistics alone at hops 128 and 16 -- 2^20 windows;
  * VT-CNN2 bf16 and the 3-filter deployed net (f32): mdc_forward_iq_u8 (bytes read by the forward kernels) against the
    normalised two-call path (mdc_iq_u8_windows_norm + mdc_forward through predict_iq_u8(normalize="rms")).

Writes profiles/iq_norm_timing.json (or --out).  Run it under `timeout`; it needs the GPU and has no fallback.
    timeout -k 10 600 python tools/time_iq_norm.py [--windows 1048576] [--reps 30] [--out profiles/iq_norm_timing.json] [--lib PATH]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from modulationdetectioncnn_amd import VTCNN2, Topology, _cabi      # noqa: E402

HBM_PEAK = 8.0e12      # bytes/s, DESIGN.md's roof


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iq_norm_timing.json"))
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
    iq = torch.randint(0, 256, (n * 256,), dtype=torch.uint8, device="cuda")
    x = torch.empty((n, 2, 128), dtype=torch.float32, device="cuda")
    st = torch.empty((n, 4), dtype=torch.int32, device="cuda")
    n16 = (n * 128 - 128) // 16 + 1      # windows of the same capture at hop 16
    st16 = torch.empty((n16, 4), dtype=torch.int32, device="cuda")
    out = {"device": torch.cuda.get_device_name(0), "windows": n, "reps": a.reps, "method": "HIP events around one launch, median of reps after 5 warm-up launches",
           "kernels": {}, "nets": {}}

    def kernel(name, fn, windows, bytes_per_window):
        med, lo, hi = median_ms(fn, a.reps)
        out["kernels"][name] = {"median_ms": med, "min_ms": lo, "max_ms": hi, "windows": windows, "bytes_per_window": bytes_per_window,
                                "TB_per_s": windows * bytes_per_window / (med * 1e-3) / 1e12,
                                "fraction_of_hbm_peak": windows * bytes_per_window / (med * 1e-3) / HBM_PEAK}
        print(name, out["kernels"][name], flush=True)

    p, xp, sp = iq.data_ptr(), x.data_ptr(), st.data_ptr()
    kernel("mdc_iq_u8_windows hop 128", lambda: _cabi.check(L.mdc_iq_u8_windows(p, n, 128, 1.0 / 127.5, xp, stream)), n, 1280)
    kernel("norm frames+stats hop 128", lambda: _cabi.check(L.mdc_iq_u8_windows_norm(p, n, 128, 7.8e-3, 1, xp, sp, stream)), n, 1296)
    kernel("norm frames hop 128", lambda: _cabi.check(L.mdc_iq_u8_windows_norm(p, n, 128, 7.8e-3, 1, xp, None, stream)), n, 1280)
    kernel("norm stats hop 128", lambda: _cabi.check(L.mdc_iq_u8_windows_norm(p, n, 128, 7.8e-3, 1, None, sp, stream)), n, 272)
    kernel("norm stats hop 16", lambda: _cabi.check(L.mdc_iq_u8_windows_norm(p, n16, 16, 7.8e-3, 1, None, st16.data_ptr(), stream)), n16, 48)
    # once more at the end: the yardstick under the clocks the others ran at
    kernel("mdc_iq_u8_windows hop 128 (again)", lambda: _cabi.check(L.mdc_iq_u8_windows(p, n, 128, 1.0 / 127.5, xp, stream)), n, 1280)
    k = out["kernels"]
    yard = min(k["mdc_iq_u8_windows hop 128"]["median_ms"], k["mdc_iq_u8_windows hop 128 (again)"]["median_ms"])
    out["frames_plus_stats_over_yardstick"] = k["norm frames+stats hop 128"]["median_ms"] / yard
    print("frames + stats / yardstick:", out["frames_plus_stats_over_yardstick"], flush=True)
    del x, st, st16

    for name, model in (("vtcnn2 bf16", VTCNN2.synthetic(Topology.vtcnn2(11), seed=2016, dtype="bf16")),
                        ("deployed3 f32", VTCNN2.synthetic("deployed3", seed=2016))):
        fused = median_ms(lambda: model.predict_iq_u8(iq, 0.02 / 127.5), a.reps, warmup=3)
        norm = median_ms(lambda: model.predict_iq_u8(iq, normalize="rms"), a.reps, warmup=3)
        out["nets"][name] = {"mdc_forward_iq_u8_median_ms": fused[0], "normalised_two_calls_median_ms": norm[0], "ratio": norm[0] / fused[0],
                             "chunk_frames": min(model.default_chunk, n)}
        print(name, out["nets"][name], flush=True)
        model._release()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
