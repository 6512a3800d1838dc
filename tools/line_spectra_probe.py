#!/usr/bin/env python3
"""What it costs to estimate the symbol rate and carrier of K detections: the batched entries (frontend.extract ->
frontend.line_spectra -> frontend.find_lines, one transfer of 48 bytes per spectrum) against the loop of the entry points that
were there before them (per stretch: frontend.ddc, three frontend.line_spectrum calls, the float64 mean, the spectrum transfer,
frontend.find_line) -- the same work, the same numbers.

A synthetic ci16 capture of 2^22 pairs and K = 7, 256 stretches (seeded starts; they may overlap) of 58,450 pairs, each isolated
at D0 = 5 with frontend.plan_taps(1, 5) into 11,683 pairs: the shape of a hopper's dwell.  Line spectra at nfft 1024, hop 512,
avg 8 (2 rows per stretch and order), orders 0, 2, 4; the bands are detect_iq(refine=True)'s for a width of 43 bins.  Three
measurements, all in this one process:

  1. (a) batched against (b) loop: device events around one whole estimate, host code included (the loop's transfers
     synchronise; so does the batched form's one transfer), `reps` estimates after a warm-up, the two forms alternating; median,
     min and max, spread = (max - min) / median.  The two forms' lines are compared first: equal to the bit, or the probe stops.
  2. the calls alone on the prepared block of isolations: mdc_iq_line_spectra (its row launches and the means) and
     mdc_iq_find_lines, device events around `reps` calls, against each kernel's bounds:
       rows    HBM: 4 bytes per isolated pair and order + 4 nfft bytes per row; LDS: per segment one staged image and a read
               and a write of it per stored pass, 8 bytes per element (the kernel's own traffic: DESIGN.md 5.17), at 128 B/clk
               per CU; issue: 5 nfft log2(nfft) flops per segment at the vector f32 peak;
       means   HBM: 4 nfft bytes per row read + 8 nfft bytes per (job, order) written;
       search  HBM: 8 nfft bytes per spectrum read; LDS: the bitonic sort's log2(nfft) (log2(nfft) + 1) / 2 stages, each a read
               and a write of nfft 8-byte keys.
     The time of the two calls cannot be split per kernel with events; --trace-hint prints the rocprofv3 line that does.

Needs the GPU; prints tables and one JSON line.

    python tools/line_spectra_probe.py [--log2-pairs 22] [--reps 20] [--boxes 7,256] [--out FILE] [--lib PATH]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_COPY_BYTES_PER_S = 6.29e12
LDS_BYTES_PER_S = 256 * 128 * 2.4e9
VALU_F32_FLOPS_PER_S = 157.3e12
D0, STRETCH, NFFT, AVG, ORDERS = 5, 58450, 1024, 8, (0, 2, 4)
BANDWIDTH = 43 / 1024


def spread(times):
    return (max(times) - min(times)) / float(np.median(times))


def summary(times):
    return dict(median_s=float(np.median(times)), min_s=min(times), max_s=max(times), spread=spread(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-pairs", type=int, default=22)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--boxes", default="7,256")
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    ap.add_argument("--trace-hint", action="store_true", help="print the profiler command that splits the calls' time per kernel, and exit")
    ap.add_argument("--lib", default=None, help="time this build of libmdc.so instead of the tree's (an A/B against a saved library)")
    a = ap.parse_args()
    if a.trace_hint:
        print("rocprofv3 --kernel-trace --stats -d profile_out -- python tools/line_spectra_probe.py --reps 5")
        return
    import torch
    from modulationdetectioncnn_amd import _cabi, frontend as F
    if not torch.cuda.is_available():
        raise SystemExit("line_spectra_probe needs the GPU: a CPU run says nothing about speed")
    if a.reps < 20:
        print(f"note: {a.reps} repetitions; the figures quoted in DESIGN.md 5.23 want at least 20")
    P = 1 << a.log2_pairs
    if a.lib:
        _cabi.LIB_PATHS["product"] = os.path.abspath(a.lib)      # before the first use: lib() loads once
    lib = _cabi.lib()
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(1)
    iq = torch.randint(-2000, 2001, (2 * P,), dtype=torch.int16, device="cuda", generator=g)
    taps = F.plan_taps(1, D0)
    b = BANDWIDTH * D0
    m = min(b / 8.0, 0.12)
    bands = [(b / 2.5, min(0.45, 1.25 * b), False), (0.0, 2.0 * m, True), (0.0, 4.0 * m, True)]
    log2n = int(np.log2(NFFT))
    forms, calls = [], []
    for K in [int(k) for k in a.boxes.split(",")]:
        starts = np.sort(np.random.default_rng(K).integers(0, P - STRETCH, size=K)).tolist()
        centres = np.random.default_rng(K + 1).uniform(-0.45, 0.45, size=K).tolist()

        def batched():
            block, offsets = F.extract(iq, "ci16", [(s, s + STRETCH, -c, 1, D0, taps) for s, c in zip(starts, centres)], whole_frames=False)
            means, _ = F.line_spectra(block.reshape(-1), "ci16", offsets, ORDERS, nfft=NFFT, avg=AVG)
            return F.find_lines(means.reshape(-1, NFFT), bands * K)

        def loop():
            out = []
            for s, c in zip(starts, centres):
                iso = F.ddc(iq[2 * s:2 * (s + STRETCH)], "ci16", shift=-c, decimate=D0, taps=taps).reshape(-1)
                for order, band in zip(ORDERS, bands):
                    rows = F.line_spectrum(iso, "ci16", order, nfft=NFFT, avg=AVG).cpu().numpy()      # the spectrum's transfer
                    acc = np.zeros(NFFT)
                    for r in range(rows.shape[0]):                                                    # the mean, in row order
                        acc += rows[r].astype(np.float64)
                    out.append(F.find_line(acc / rows.shape[0], *band))
            return out

        variants = {"batched": batched, "loop": loop}
        first = {name: fn() for name, fn in variants.items()}      # warm-up: code objects, allocator, the cached window
        if first["batched"] != first["loop"]:
            raise SystemExit(f"K = {K}: the batched lines and the loop's differ")
        for fn in variants.values():
            fn()
        times = {name: [] for name in variants}
        for _ in range(a.reps):
            for name, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e-3)
        row = dict(boxes=K, lines=len(first["batched"]))
        for name, ts in times.items():
            row.update({f"{name}_{k}": v for k, v in summary(ts).items()})
        row["loop_over_batched"] = row["loop_median_s"] / row["batched_median_s"]
        # faster by more than the spread of the repetitions: the slowest batched estimate against the fastest loop
        row["batched_faster_beyond_spread"] = bool(row["batched_max_s"] < row["loop_min_s"])
        forms.append(row)

        # the two calls alone on the prepared block
        block, offsets = F.extract(iq, "ci16", [(s, s + STRETCH, -c, 1, D0, taps) for s, c in zip(starts, centres)], whole_frames=False)
        flat = block.reshape(-1)
        pairs = int(offsets[-1])
        rec = np.zeros(K, _cabi.IQ_LINE_JOB)
        rec["first_pair"], rec["pairs"] = offsets[:-1], np.diff(offsets)
        total = _cabi.check(lib.mdc_iq_line_spectra_rows(rec.ctypes.data, K, pairs, NFFT, NFFT // 2, AVG))
        jobs_dev = torch.from_numpy(rec.view(np.int64).reshape(K, 4)).cuda()
        w, scale = F._default_window(NFFT, iq.device)
        rows = torch.empty((3, total, NFFT), dtype=torch.float32, device="cuda")
        means = torch.empty((K, 3, NFFT), dtype=torch.float64, device="cuda")
        orders = np.asarray(ORDERS, np.int32)
        band_rec = np.zeros(3 * K, _cabi.IQ_LINE_BAND)
        for i, (lo, hi, two) in enumerate(bands * K):
            band_rec[i] = (lo, hi, int(two), 0)
        bands_dev = torch.from_numpy(band_rec.view(np.uint8).reshape(3 * K, -1)).cuda()
        records = torch.empty((3 * K, _cabi.IQ_LINE_RECORD.itemsize), dtype=torch.uint8, device="cuda")

        def spectra():
            _cabi.check(lib.mdc_iq_line_spectra(flat.data_ptr(), _cabi.IQ_CI16, pairs, rec.ctypes.data, jobs_dev.data_ptr(), K, orders.ctypes.data, 3, NFFT,
                                                NFFT // 2, AVG, w.data_ptr(), scale, rows.data_ptr(), total, means.data_ptr(), stream))

        def search():
            _cabi.check(lib.mdc_iq_find_lines(means.data_ptr(), 3 * K, NFFT, band_rec.ctypes.data, bands_dev.data_ptr(), records.data_ptr(), stream))

        entry = dict(boxes=K, isolated_pairs=pairs, rows_per_plane=int(total))
        for name, fn in (("line_spectra", spectra), ("find_lines", search)):
            fn()
            fn()
            torch.cuda.synchronize()
            ts = []
            for _ in range(5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    fn()
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e-3 / a.reps)
            entry.update({f"{name}_{k}": v for k, v in summary(ts).items()})
        segs = 3 * total * AVG
        stored_passes = log2n // 2 if log2n % 2 else log2n // 2 - 1
        entry["bounds_s"] = dict(
            rows_hbm=(3 * 4 * pairs + 3 * total * 4 * NFFT) / HBM_COPY_BYTES_PER_S,
            rows_lds=segs * 8 * NFFT * (1 + 2 * stored_passes + 1) / LDS_BYTES_PER_S,
            rows_issue=segs * 5 * NFFT * log2n / VALU_F32_FLOPS_PER_S,
            means_hbm=(3 * total * 4 * NFFT + 3 * K * 8 * NFFT) / HBM_COPY_BYTES_PER_S,
            search_hbm=3 * K * 8 * NFFT / HBM_COPY_BYTES_PER_S,
            search_lds=3 * K * (log2n * (log2n + 1) // 2) * 2 * 8 * NFFT / LDS_BYTES_PER_S)
        calls.append(entry)
        del block, flat, rows, means

    print(f"device: {torch.cuda.get_device_name(0)}; ci16, 2^{a.log2_pairs} pairs; stretches of {STRETCH} pairs isolated at D0 = {D0}; {a.reps} repetitions")
    print("one estimate of all stretches (ms: median [min .. max], spread)")
    print(f"{'boxes':>6s} {'batched':>36s} {'loop':>36s} {'loop / batched':>15s} {'beyond spread':>14s}")
    for r in forms:
        cell = lambda n: f"{r[n + '_median_s'] * 1e3:9.3f} [{r[n + '_min_s'] * 1e3:9.3f} .. {r[n + '_max_s'] * 1e3:9.3f}] {r[n + '_spread'] * 100:5.1f}%"      # noqa: E731
        print(f"{r['boxes']:6d} {cell('batched'):>36s} {cell('loop'):>36s} {r['loop_over_batched']:15.2f} {str(r['batched_faster_beyond_spread']):>14s}")
    print("the calls alone (us: median, spread) and their kernels' bounds (us)")
    for r in calls:
        bd = {k: v * 1e6 for k, v in r["bounds_s"].items()}
        print(f"{r['boxes']:6d} boxes, {r['rows_per_plane']} rows per plane: line_spectra {r['line_spectra_median_s'] * 1e6:9.2f} ({r['line_spectra_spread'] * 100:4.1f}%)  "
              f"find_lines {r['find_lines_median_s'] * 1e6:9.2f} ({r['find_lines_spread'] * 100:4.1f}%)")
        print("       bounds: " + "  ".join(f"{k} {v:.3f}" for k, v in bd.items()))
    out = json.dumps({"tool": "line_spectra_probe", "device": torch.cuda.get_device_name(0), "log2_pairs": a.log2_pairs, "reps": a.reps, "forms": forms,
                      "calls": calls})
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(out + "\n")


if __name__ == "__main__":
    main()
