#!/usr/bin/env python3
"""Throughput of mdc_iq_synth_frames (csrc/iq_synth.hip) on the device, next to a device-to-device copy of the bytes it writes,
timed in the same process, and the numpy restatement's rate on the host for scale.

A frame costs a few thousand integer instructions per wave (16 draws per lane for the noise alone) against 512 bytes stored: the
kernel is expected to be bound by the vector ALU, not by HBM.  Per size (2^16 and 2^20 frames) three recipes:
    rml11    the eleven classes of RML2016_MODS, twenty SNRs (synth_recipe's default)
    linear   the six alphabet + root-raised-cosine classes only
    phase    CPFSK, GFSK and WBFM only (the PHASE mode: oscillator reads and the wave scan on top of the filter)
and a copy (Tensor.copy_ between two device buffers) of the output's n * 512 bytes.  `of copy` is the copy's time over the
kernel's: 1.0 would mean frames are generated as fast as finished frames can be copied.  Then mdc_iq_synth_frames_faded on rml11:
    fade3    synth_fading's default: three paths of eight taps, gains constant over a frame
    fade4x16 four paths of sixteen taps with Doppler on: the most a fading record can ask for
`vs rml11` is the unfaded rml11 time of the same size over the row's.  --other-lib PATH times rml11 through another build of the
library too (the one saved before an edit, as tools/ab_libs.py takes it), in the same rounds: `spread` -- (max - min) / median of a
case's windows -- is the run-to-run noise a difference between the two has to exceed.

Timing: device events around `reps` back-to-back launches after a warm-up, the median of `rounds` such windows, the cases
alternating within every round.  Needs the GPU; prints a table and one JSON line.

    python tools/synth_probe.py [--log2-frames 16 20] [--rounds 5] [--reps 10] [--host-frames 2048] [--other-lib PATH] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RECIPES = {"rml11": None, "linear": ("BPSK", "QPSK", "8PSK", "PAM4", "QAM16", "QAM64"), "phase": ("CPFSK", "GFSK", "WBFM")}


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
    ap.add_argument("--log2-frames", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-frames", type=int, default=2048, help="frames of the numpy restatement timed on the host (0: skip)")
    ap.add_argument("--other-lib", default=None, help="another build of libmdc.so: rml11 is timed through it as well")
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    a = ap.parse_args()
    import torch
    from modulationdetectioncnn_amd import _cabi, frontend
    if not torch.cuda.is_available():
        raise SystemExit("synth_probe needs the GPU: a CPU run says nothing about speed")
    lib = _cabi.lib()
    stream = torch.cuda.current_stream().cuda_stream
    recipes = {name: frontend.synth_recipe() if mods is None else frontend.synth_recipe(mods=mods) for name, mods in RECIPES.items()}
    plans = {name: (np.ascontiguousarray(r.blob), torch.from_numpy(np.ascontiguousarray(r.blob)).cuda()) for name, r in recipes.items()}
    fadings = {"fade3": frontend.synth_fading(),
               "fade4x16": frontend.synth_fading(delays=(0.0, 0.5, 1.0, 1.5), mags=(1.0, 0.8, 0.5, 0.3), ntaps=16, max_doppler=0.001, kaiser_beta=8.0)}
    records = {name: np.ascontiguousarray(f.record) for name, f in fadings.items()}
    other = None
    if a.other_lib:
        _cabi.LIB_PATHS["other"] = os.path.abspath(a.other_lib)
        other = _cabi.lib("other")
    rows = []
    for lg in a.log2_frames:
        n = 1 << lg
        iq = torch.empty((n, 256), dtype=torch.int16, device="cuda")
        labels = torch.empty(n, dtype=torch.int32, device="cuda")
        snr = torch.empty(n, dtype=torch.int32, device="cuda")
        sat = torch.zeros(1, dtype=torch.int64, device="cuda")
        dst = torch.empty_like(iq)
        cases = []
        for name, (blob, plan_dev) in plans.items():

            def run(blob=blob, plan_dev=plan_dev):
                _cabi.check(lib.mdc_iq_synth_frames(blob.ctypes.data, plan_dev.data_ptr(), blob.size, 2016, 0, n, iq.data_ptr(), labels.data_ptr(),
                                                    snr.data_ptr(), sat.data_ptr(), stream))

            cases.append(dict(kernel="mdc_iq_synth_frames", recipe=name, run=run, times=[]))
        blob, plan_dev = plans["rml11"]
        for name, record in records.items():

            def run_faded(record=record):
                _cabi.check(lib.mdc_iq_synth_frames_faded(blob.ctypes.data, plan_dev.data_ptr(), blob.size, 2016, 0, n, iq.data_ptr(), labels.data_ptr(),
                                                          snr.data_ptr(), sat.data_ptr(), record.ctypes.data, stream))

            cases.append(dict(kernel="mdc_iq_synth_frames_faded", recipe=name, run=run_faded, times=[]))
        if other is not None:

            def run_other():
                _cabi.check(other.mdc_iq_synth_frames(blob.ctypes.data, plan_dev.data_ptr(), blob.size, 2016, 0, n, iq.data_ptr(), labels.data_ptr(),
                                                      snr.data_ptr(), sat.data_ptr(), stream), "other")

            cases.append(dict(kernel="other build", recipe="rml11", run=run_other, times=[]))

        def copy():
            dst.copy_(iq, non_blocking=True)

        cases.append(dict(kernel="copy", recipe="-", run=copy, times=[]))
        for c in cases:      # warm-up: code objects
            c["run"]()
            c["run"]()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for c in cases:
                c["times"].append(_time(c["run"], a.reps, torch))
        t_copy = float(np.median(cases[-1]["times"]))
        t_rml11 = float(np.median(cases[0]["times"]))
        for c in cases:
            t = float(np.median(c["times"]))
            rows.append(dict(kernel=c["kernel"], recipe=c["recipe"], log2_frames=lg, frames=n, bytes_written=512 * n, seconds=t,
                             seconds_min=float(min(c["times"])), seconds_max=float(max(c["times"])), spread=(max(c["times"]) - min(c["times"])) / t,
                             frames_per_s=n / t, gbytes_written_per_s=512 * n / t / 1e9, of_copy=t_copy / t, vs_rml11=t_rml11 / t))
        del iq, dst, cases
        torch.cuda.empty_cache()
    host = None
    if a.host_frames > 0:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import iq_synth_ref
        r = recipes["rml11"]
        t0 = time.perf_counter()
        iq_synth_ref.synth(r.classes, r.points, r.taps, r.gain_sig, r.gain_noise, r.max_step, r.q, 2016, 0, a.host_frames)
        host = dict(frames=a.host_frames, seconds=time.perf_counter() - t0)
        host["frames_per_s"] = host["frames"] / host["seconds"]
    print(f"device: {torch.cuda.get_device_name(0)}; median of {a.rounds} windows of {a.reps} launches")
    print(f"{'kernel':26s} {'recipe':8s} {'frames':>6s} {'ms':>9s} {'Mframes/s':>10s} {'GB/s out':>9s} {'of copy':>8s} {'vs rml11':>8s} {'spread':>7s}")
    for r in rows:
        print(f"{r['kernel']:26s} {r['recipe']:8s} {'2^%d' % r['log2_frames']:>6s} {r['seconds'] * 1e3:9.4f} {r['frames_per_s'] / 1e6:10.2f} "
              f"{r['gbytes_written_per_s']:9.1f} {r['of_copy']:8.2f} {r['vs_rml11']:8.2f} {r['spread']:7.3f}")
    if host:
        print(f"numpy restatement on the host, rml11: {host['frames_per_s']:.0f} frames/s ({host['frames']} frames)")
    out_rec = json.dumps({"tool": "synth_probe", "device": torch.cuda.get_device_name(0), "rows": rows, "host_restatement": host})
    print(out_rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(out_rec + "\n")


if __name__ == "__main__":
    main()
