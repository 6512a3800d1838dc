#!/usr/bin/env python3
"""What VTCNN2.detect_iq costs BEHIND its search, per-detection loop against batched=True, and the throughput of mdc_iq_extract
(csrc/iq_extract.hip) alone.

A synthetic ci16 capture of 2^24 pairs and K = 8, 64, 512, 4096 boxes (seeded: starts anywhere, 2,048 .. 32,768 pairs long,
log-uniform; bandwidths from a list that frontend.channel_plan turns into a mix of (L, D), integer decimations among them).
Three measurements, all in this one process:

  1. detect_iq(batched=False) and detect_iq(batched=True) behind the search.  The search is taken out of BOTH the same way:
     while a call is timed, frontend.spectrogram / detection_threshold / find_detections are replaced by functions that return
     a one-row spectrogram made beforehand and the K prepared boxes -- so the timed code is the package's own, line for line,
     from the first channel_plan to the returned records.  Host clock around the call plus a device synchronise; the two
     variants alternate within every round; median, min and max of the rounds, spread = (max - min) / median.  For K <= 512 the
     two record lists are compared first: equal key for key and bit for bit, or the probe stops.
  2. The extract kernel alone on each K's plan (plan and its device copy made once): device events around `reps` launches, median
     of the rounds; input pairs/s, and the share of the nearer roof -- the larger of the HBM bound (4 bytes per input pair of every
     job, read once per job, + 4 bytes per output pair, at the measured copy rate of 6.29 TB/s) and the packed-dot-product bound
     (2 * ceil(B / 2) lane-operations per output pair, B = ceil(T / L), on 256 CUs x 4 SIMDs x 32 lanes/clk at 2.4 GHz) over the
     time: the roofs of tools/resample_probe.py.
  3. One job spanning the whole capture at (L, D) in {(1, 12), (5, 6), (25, 32)}: mdc_iq_extract against mdc_iq_resample on the
     same arguments, alternating, the same bits asserted -- what calling the shared mix_tile / fir_output and reading the job,
     the filter and the taps from memory cost against the resampler's private copies and by-value taps.

Needs the GPU; prints tables and one JSON line.

    python tools/extract_probe.py [--log2-pairs 24] [--rounds 5] [--reps 10] [--boxes 8,64,512,4096] [--out FILE]
"""
import argparse
import json
import os
import sys
import time
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_COPY_BYTES_PER_S = 6.29e12
VALU_LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9
BANDWIDTHS = [0.0125, 0.02, 0.03375, 0.05, 0.084375, 0.1, 0.16875, 0.2]      # 0.03375 / 0.084375 / 0.16875: D = 5, 2, 1 exactly
WHOLE_SHAPES = [(1, 12), (5, 6), (25, 32)]
Detection = namedtuple("Detection", "first_row stop_row first_bin stop_bin cells centre bandwidth peak_db snr_db first_pair stop_pair")


def boxes(K, pairs, seed):
    rng = np.random.default_rng(seed)
    length = np.exp(rng.uniform(np.log(2048), np.log(32768), K)).astype(np.int64)
    first = rng.integers(0, pairs - length)
    out = [Detection(0, 1, 0, 1, 1, float(rng.uniform(-0.45, 0.45)), BANDWIDTHS[int(rng.integers(len(BANDWIDTHS)))], 0.0, 0.0, int(a), int(a + n))
           for a, n in zip(first, length)]
    out.sort(key=lambda d: (d.first_pair, d.centre))
    return out


class search_replaced:
    """frontend's three search calls return prepared values while this is active (see the module's text)"""

    def __init__(self, F, spec, found):
        self.F, self.spec, self.found = F, spec, found

    def __enter__(self):
        F = self.F
        self.saved = F.spectrogram, F.detection_threshold, F.find_detections
        F.spectrogram = lambda *a, **k: self.spec
        F.detection_threshold = lambda *a, **k: None
        F.find_detections = lambda *a, **k: self.found

    def __exit__(self, *exc):
        self.F.spectrogram, self.F.detection_threshold, self.F.find_detections = self.saved


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


def same_records(x, y, torch):
    if len(x) != len(y):
        return False
    for b, r in zip(x, y):
        if list(b) != list(r):
            return False
        for k in r:
            if not (torch.equal(b[k], r[k]) if isinstance(r[k], torch.Tensor) else b[k] == r[k]):
                return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-pairs", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--boxes", default="8,64,512,4096")
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    ap.add_argument("--kernel-only", action="store_true", help="skip measurement 1 (the detector): the kernel rows alone, for an A/B of two builds")
    ap.add_argument("--lib", default=None, help="time this build of libmdc.so instead of the tree's (an A/B against a saved library)")
    a = ap.parse_args()
    import torch
    from modulationdetectioncnn_amd import VTCNN2, _cabi, frontend as F
    if not torch.cuda.is_available():
        raise SystemExit("extract_probe needs the GPU: a CPU run says nothing about speed")
    P = 1 << a.log2_pairs
    if a.lib:
        _cabi.LIB_PATHS["product"] = os.path.abspath(a.lib)      # before the first use: lib() loads once
    lib = _cabi.lib()
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(1)
    iq = torch.randint(-2000, 2001, (2 * P,), dtype=torch.int16, device="cuda", generator=g)
    model = VTCNN2.synthetic("deployed3")
    spec = torch.ones((1, 1024), dtype=torch.float32, device="cuda")
    detect, kernel = [], []
    for K in [int(k) for k in a.boxes.split(",")]:
        found = boxes(K, P, seed=K)
        if not a.kernel_only:
            with search_replaced(F, spec, found):
                variants = {"loop": lambda: model.detect_iq(iq, "ci16", batched=False), "batched": lambda: model.detect_iq(iq, "ci16", batched=True)}
                first = {name: fn() for name, fn in variants.items()}      # warm-up: code objects, allocator, tap designs
                checked = K <= 512
                if checked and not same_records(first["batched"], first["loop"], torch):
                    raise SystemExit(f"K = {K}: batched and loop records differ")
                windows = sum(r["windows"] for r in first["batched"])
                del first
                times = {name: [] for name in variants}
                for _ in range(a.rounds):
                    for name, fn in variants.items():
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fn()
                        torch.cuda.synchronize()
                        times[name].append(time.perf_counter() - t0)
            row = dict(boxes=K, windows=windows, records_compared=checked)
            for name, ts in times.items():
                row.update({f"{name}_s": float(np.median(ts)), f"{name}_min_s": min(ts), f"{name}_max_s": max(ts), f"{name}_spread": spread(ts)})
            row["loop_over_batched"] = row["loop_s"] / row["batched_s"]
            detect.append(row)
        # the kernel alone on this K's plan
        taps, stretches = {}, []
        for d, (shift, L, D, _) in zip(found, F.channel_plans([(d.centre, d.bandwidth) for d in found])):
            if (L, D) not in taps:
                taps[L, D] = F.plan_taps(L, D)
            h = taps[L, D]
            stretches.append((d.first_pair, d.stop_pair - d.first_pair, 0, F.phase_step(shift), (L, D),
                              lib.mdc_iq_resample_out_count(d.stop_pair - d.first_pair, h.size, L, D) // 128 * 128))
        order = list(taps)
        blob, out_pairs = F.extract_plan([s[:4] + (order.index(s[4]), s[5]) for s in stretches], [(L, D, taps[L, D]) for L, D in order], "ci16", P)
        plan_dev, out = torch.from_numpy(blob).cuda(), torch.empty((out_pairs, 2), dtype=torch.int16, device="cuda")

        def run(blob=blob, plan_dev=plan_dev, out=out, out_pairs=out_pairs):
            _cabi.check(lib.mdc_iq_extract(iq.data_ptr(), _cabi.IQ_CI16, P, blob.ctypes.data, plan_dev.data_ptr(), blob.size, out.data_ptr(), out_pairs, stream))

        run()
        run()
        torch.cuda.synchronize()
        ts = [event_time(run, a.reps, torch) for _ in range(a.rounds)]
        t = float(np.median(ts))
        pairs = sum(s[1] for s in stretches)
        nbytes = 4 * pairs + 4 * out_pairs
        dot_ops = sum(2 * ((-(-taps[s[4]].size // s[4][0]) + 1) // 2) * s[5] for s in stretches)
        ntiles = int(blob[24:32].view(np.int64)[0])
        kernel.append(dict(boxes=K, filters=len(order), tiles=ntiles, pairs_in=pairs, out_pairs=out_pairs, plan_bytes=int(blob.size), seconds=t,
                           seconds_min=min(ts), seconds_max=max(ts), spread=spread(ts), pairs_per_s=pairs / t, gbytes_per_s=nbytes / t / 1e9,
                           hbm_bound_s=nbytes / HBM_COPY_BYTES_PER_S, dot2_bound_s=dot_ops / VALU_LANE_OPS_PER_S,
                           nearer_roof="hbm" if nbytes / HBM_COPY_BYTES_PER_S >= dot_ops / VALU_LANE_OPS_PER_S else "dot2",
                           share_of_bound=max(nbytes / HBM_COPY_BYTES_PER_S, dot_ops / VALU_LANE_OPS_PER_S) / t))
        del plan_dev, out
    # one job over the whole capture: mdc_iq_extract against mdc_iq_resample
    whole = []
    step = F.phase_step(-0.2)
    for L, D in WHOLE_SHAPES:
        h = F.design_resampler(L, D)
        n_out = lib.mdc_iq_resample_out_count(P, h.size, L, D)
        blob, out_pairs = F.extract_plan([(0, P, 0, step, 0, n_out)], [(L, D, h)], "ci16", P)
        plan_dev = torch.from_numpy(blob).cuda()
        o_ext, o_res = (torch.empty((n_out, 2), dtype=torch.int16, device="cuda") for _ in range(2))

        def ext(blob=blob, plan_dev=plan_dev, o=o_ext, n=n_out):
            _cabi.check(lib.mdc_iq_extract(iq.data_ptr(), _cabi.IQ_CI16, P, blob.ctypes.data, plan_dev.data_ptr(), blob.size, o.data_ptr(), n, stream))

        def res(L=L, D=D, h=h, o=o_res, n=n_out):
            _cabi.check(lib.mdc_iq_resample(iq.data_ptr(), _cabi.IQ_CI16, P, 0, step, L, D, h.ctypes.data, h.size, o.data_ptr(), n, stream))

        for fn in (ext, res, ext, res):
            fn()
        torch.cuda.synchronize()
        assert torch.equal(o_ext, o_res)
        te, tr = [], []
        for _ in range(a.rounds):
            te.append(event_time(ext, a.reps, torch))
            tr.append(event_time(res, a.reps, torch))
        whole.append(dict(interpolate=L, decimate=D, ntaps=int(h.size), pairs=P, n_out=n_out, extract_s=float(np.median(te)), extract_spread=spread(te),
                          resample_s=float(np.median(tr)), resample_spread=spread(tr), extract_over_resample=float(np.median(te) / np.median(tr))))
    model._release()

    print(f"device: {torch.cuda.get_device_name(0)}; ci16, 2^{a.log2_pairs} pairs; {a.rounds} rounds (kernel rows: windows of {a.reps} launches)")
    if detect:
        print("detect_iq behind the search (ms: median [min .. max], spread)")
        print(f"{'boxes':>6s} {'windows':>8s} {'loop':>34s} {'batched':>34s} {'loop / batched':>15s}")
    for r in detect:
        cell = lambda n: f"{r[n + '_s'] * 1e3:9.3f} [{r[n + '_min_s'] * 1e3:8.3f} .. {r[n + '_max_s'] * 1e3:8.3f}] {r[n + '_spread'] * 100:4.1f}%"      # noqa: E731
        print(f"{r['boxes']:6d} {r['windows']:8d} {cell('loop'):>34s} {cell('batched'):>34s} {r['loop_over_batched']:15.2f}")
    print("mdc_iq_extract alone")
    print(f"{'boxes':>6s} {'filters':>7s} {'tiles':>6s} {'Mpairs in':>10s} {'ms':>8s} {'spread':>7s} {'Gpairs/s':>9s} {'GB/s':>8s} {'HBM ms':>8s} {'dot2 ms':>8s} {'of bound':>9s}")
    for r in kernel:
        print(f"{r['boxes']:6d} {r['filters']:7d} {r['tiles']:6d} {r['pairs_in'] / 1e6:10.2f} {r['seconds'] * 1e3:8.3f} {r['spread'] * 100:6.1f}% "
              f"{r['pairs_per_s'] / 1e9:9.2f} {r['gbytes_per_s']:8.1f} {r['hbm_bound_s'] * 1e3:8.3f} {r['dot2_bound_s'] * 1e3:8.3f} {r['share_of_bound']:9.2f}")
    print("one job over the whole capture")
    print(f"{'L':>3s} {'D':>3s} {'T':>4s} {'extract ms':>11s} {'spread':>7s} {'resample ms':>12s} {'spread':>7s} {'extract / resample':>19s}")
    for r in whole:
        print(f"{r['interpolate']:3d} {r['decimate']:3d} {r['ntaps']:4d} {r['extract_s'] * 1e3:11.3f} {r['extract_spread'] * 100:6.1f}% "
              f"{r['resample_s'] * 1e3:12.3f} {r['resample_spread'] * 100:6.1f}% {r['extract_over_resample']:19.3f}")
    rec = json.dumps({"tool": "extract_probe", "device": torch.cuda.get_device_name(0), "log2_pairs": a.log2_pairs, "rounds": a.rounds, "reps": a.reps,
                      "detect_iq_behind_search": detect, "extract_kernel": kernel, "whole_capture_job": whole})
    print(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(rec + "\n")


if __name__ == "__main__":
    main()
