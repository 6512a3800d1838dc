#!/usr/bin/env python3
"""Throughput of mdc_iq_synth_capture (csrc/iq_synth_capture.hip) on the device, next to a device-to-device copy of the bytes it
writes, timed in the same process, and the numpy restatement's rate on the host for scale.

Per size (2^24 and 2^27 capture pairs) three scenes over the eleven classes of RML2016_MODS:
    noise    no emitter: the noise draws (32 per lane), the rounding shift and the store alone
    cont8    eight continuous emitters (one of them GFSK: the PHASE pre-pass runs), 8 .. 32 samples per symbol
    duty32   32 emitters, each on for 10 % of its period, the periods a few tiles long and staggered: most (emitter, tile) pairs
             are skipped by the gate
and a copy (Tensor.copy_ between two device buffers) of the output's 4 n bytes.  `of copy` is the copy's time over the kernel's.

Timing: device events around `reps` back-to-back calls after a warm-up, the median of `rounds` such windows, the cases
alternating within every round.  Needs the GPU; prints a table and one JSON line.

    python tools/scene_probe.py [--log2-pairs 24 27] [--rounds 5] [--reps 4] [--host-pairs 65536] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

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


def scenes(frontend):
    recipe = frontend.synth_recipe()
    mods = frontend.RML2016_MODS
    cont8 = [dict(mod=m, samples_per_symbol=sps, centre=c, level_db=15.0)
             for m, sps, c in zip(("QPSK", "BPSK", "GFSK", "8PSK", "QAM16", "AM-DSB", "PAM4", "QAM64"), (8, 12, 16, 16, 24, 32, 32, 20),
                                  np.linspace(-0.42, 0.42, 8))]
    duty32 = [dict(mod=mods[k % len(mods)], samples_per_symbol=(8, 16, 32)[k % 3], centre=(k - 15.5) / 34.0, level_db=15.0, start=1000 * k,
                   on=2000 + 50 * k, period=20000 + 500 * k) for k in range(32)]
    return {"noise": frontend.synth_scene(recipe, [], 300.0), "cont8": frontend.synth_scene(recipe, cont8, 300.0),
            "duty32": frontend.synth_scene(recipe, duty32, 300.0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-pairs", type=int, nargs="+", default=[24, 27])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--host-pairs", type=int, default=65536, help="pairs of the numpy restatement timed on the host per scene (0: skip)")
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    a = ap.parse_args()
    import torch
    from modulationdetectioncnn_amd import _cabi, frontend
    if not torch.cuda.is_available():
        raise SystemExit("scene_probe needs the GPU: a CPU run says nothing about speed")
    lib = _cabi.lib()
    stream = torch.cuda.current_stream().cuda_stream
    built = scenes(frontend)
    plan = np.ascontiguousarray(next(iter(built.values())).recipe.blob)
    plan_dev = torch.from_numpy(plan).cuda()
    rows = []
    for lg in a.log2_pairs:
        n = 1 << lg
        out = torch.empty(2 * n, dtype=torch.int16, device="cuda")
        dst = torch.empty_like(out)
        sat = torch.zeros(1, dtype=torch.int64, device="cuda")
        cases = []
        for name, scene in built.items():
            blob = np.ascontiguousarray(scene.blob)
            blob_dev = torch.from_numpy(blob).cuda()
            wbytes = _cabi.check(lib.mdc_iq_synth_capture_workspace_bytes(blob.ctypes.data, blob.size, n))
            work = torch.empty(max(wbytes, 16), dtype=torch.uint8, device="cuda")

            def run(blob=blob, blob_dev=blob_dev, work=work, wbytes=wbytes):
                _cabi.check(lib.mdc_iq_synth_capture(blob.ctypes.data, blob_dev.data_ptr(), blob.size, plan.ctypes.data, plan_dev.data_ptr(), plan.size,
                                                     2016, n, out.data_ptr(), sat.data_ptr(), work.data_ptr(), wbytes, stream))

            cases.append(dict(kernel="mdc_iq_synth_capture", scene=name, run=run, times=[]))

        def copy():
            dst.copy_(out, non_blocking=True)

        cases.append(dict(kernel="copy", scene="-", run=copy, times=[]))
        for c in cases:      # warm-up: code objects
            c["run"]()
            c["run"]()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for c in cases:
                c["times"].append(_time(c["run"], a.reps, torch))
        t_copy = float(np.median(cases[-1]["times"]))
        for c in cases:
            t = float(np.median(c["times"]))
            rows.append(dict(kernel=c["kernel"], scene=c["scene"], log2_pairs=lg, pairs=n, bytes_written=4 * n, seconds=t,
                             seconds_min=float(min(c["times"])), seconds_max=float(max(c["times"])), spread=(max(c["times"]) - min(c["times"])) / t,
                             pairs_per_s=n / t, gbytes_written_per_s=4 * n / t / 1e9, of_copy=t_copy / t))
        del out, dst, cases
        torch.cuda.empty_cache()
    host = []
    if a.host_pairs > 0:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import iq_synth_capture_ref
        for name, scene in built.items():
            t0 = time.perf_counter()
            iq_synth_capture_ref.scene_capture(scene, 2016, a.host_pairs)
            dt = time.perf_counter() - t0
            host.append(dict(scene=name, pairs=a.host_pairs, seconds=dt, pairs_per_s=a.host_pairs / dt))
    print(f"device: {torch.cuda.get_device_name(0)}; median of {a.rounds} windows of {a.reps} calls")
    print(f"{'kernel':22s} {'scene':7s} {'pairs':>6s} {'ms':>10s} {'Gpairs/s':>9s} {'GB/s out':>9s} {'of copy':>8s} {'spread':>7s}")
    for r in rows:
        print(f"{r['kernel']:22s} {r['scene']:7s} {'2^%d' % r['log2_pairs']:>6s} {r['seconds'] * 1e3:10.4f} {r['pairs_per_s'] / 1e9:9.3f} "
              f"{r['gbytes_written_per_s']:9.1f} {r['of_copy']:8.3f} {r['spread']:7.3f}")
    for h in host:
        print(f"numpy restatement on the host, {h['scene']}: {h['pairs_per_s']:.0f} pairs/s ({h['pairs']} pairs)")
    out_rec = json.dumps({"tool": "scene_probe", "device": torch.cuda.get_device_name(0), "rows": rows, "host_restatement": host})
    print(out_rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(out_rec + "\n")


if __name__ == "__main__":
    main()
