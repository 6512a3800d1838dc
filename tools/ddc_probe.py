#!/usr/bin/env python3
"""Throughput of mdc_iq_ddc (frequency shift + low-pass + decimate, csrc/iq_ddc.hip) on the device, next to a plain torch
statement of the same chain as the yardstick.

For CU8 and CI16 at (D, T) in {(4, 32), (12, 96), (64, 512)} on 2^26 input pairs: input pairs/s and GB/s (the bytes the
algorithm needs: pair_bytes per input pair read once + 4 bytes per output pair written), the share of the HBM bound those bytes
set at the measured copy rate of the MI355X (6.29 TB/s), and the packed-dot-product bound (2 * ceil(T/2) / D lane-operations per
input pair on 256 CUs x 4 SIMDs x 32 lanes/clk at 2.4 GHz).  The yardstick, in the same run on the same data: the capture as
complex64, one complex multiply by the oscillator, then torch.nn.functional.conv1d with stride D on the real and imaginary
rows in f32 (its conversion from the integer capture is not timed: only multiply + filter are).

Timing: device events around `reps` back-to-back launches after a warm-up, the median of `rounds` such windows, mdc_iq_ddc and
the yardstick alternating.  Needs the GPU; prints a table and one JSON line.

    python tools/ddc_probe.py [--log2-pairs 26] [--rounds 5] [--reps 10] [--out FILE] [--lib PATH]
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
SHAPES = [(4, 32), (12, 96), (64, 512)]


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
        raise SystemExit("ddc_probe needs the GPU: a CPU run says nothing about speed")
    P = 1 << a.log2_pairs
    if a.lib:
        _cabi.LIB_PATHS["product"] = os.path.abspath(a.lib)      # before the first use: lib() loads once
    L = _cabi.lib()
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(1)
    rows = []
    for fmt, name, dt, lo, hi in ((_cabi.IQ_CU8, "cu8", torch.uint8, 0, 256), (_cabi.IQ_CI16, "ci16", torch.int16, -32768, 32768)):
        iq = torch.randint(lo, hi, (2 * P,), dtype=dt, device="cuda", generator=g)
        pair_bytes = _cabi.IQ_PAIR_BYTES[fmt]
        # the yardstick's input: complex64 samples at 16-bit full scale (conversion not timed)
        f = iq.to(torch.float32).view(-1, 2)
        f = (2.0 * f - 255.0) * 128.0 if fmt == _cabi.IQ_CU8 else f
        z = torch.complex(f[:, 0].contiguous(), f[:, 1].contiguous())
        del f
        step = frontend.phase_step(-0.2)
        osc = torch.polar(torch.ones(P, device="cuda"), (2.0 * np.pi * (-0.2)) * torch.arange(P, device="cuda", dtype=torch.float32))
        for D, T in SHAPES:
            h = frontend.design_lowpass(D, ntaps=T)
            n_out = L.mdc_iq_ddc_out_count(P, T, D)
            out = torch.empty((n_out, 2), dtype=torch.int16, device="cuda")
            w = torch.from_numpy(h.astype(np.float32) / 32768.0).cuda().view(1, 1, T)

            def ours():
                _cabi.check(L.mdc_iq_ddc(iq.data_ptr(), fmt, P, 0, step, D, h.ctypes.data, T, out.data_ptr(), n_out, stream))

            def torch_chain():
                m = torch.view_as_real(z * osc).t().contiguous().view(2, 1, P)
                return torch.nn.functional.conv1d(m, w, stride=D)

            for fn in (ours, torch_chain):      # warm-up: code objects, algorithm choice, allocator
                fn()
                fn()
            torch.cuda.synchronize()
            t_ours, t_torch = [], []
            for _ in range(a.rounds):
                t_ours.append(_time(ours, a.reps, torch))
                t_torch.append(_time(torch_chain, max(1, a.reps // 5), torch))
            to, tt = float(np.median(t_ours)), float(np.median(t_torch))
            nbytes = pair_bytes * P + 4 * n_out
            dot_ops = 2 * ((T + 1) // 2) / D * P
            bound = max(nbytes / HBM_COPY_BYTES_PER_S, dot_ops / VALU_LANE_OPS_PER_S)
            rows.append(dict(format=name, decimate=D, ntaps=T, pairs=P, seconds=to, seconds_min=float(min(t_ours)), pairs_per_s=P / to,
                             gbytes_per_s=nbytes / to / 1e9, hbm_bound_s=nbytes / HBM_COPY_BYTES_PER_S, dot2_bound_s=dot_ops / VALU_LANE_OPS_PER_S,
                             share_of_bound=bound / to, torch_seconds=tt, torch_pairs_per_s=P / tt, speedup_over_torch=tt / to))
            del out, w
        del iq, z, osc
        torch.cuda.empty_cache()
    print(f"device: {torch.cuda.get_device_name(0)}; 2^{a.log2_pairs} input pairs; median of {a.rounds} windows of {a.reps} launches")
    print(f"{'fmt':5s} {'D':>3s} {'T':>4s} {'ms':>8s} {'Gpairs/s':>9s} {'GB/s':>8s} {'HBM bound ms':>13s} {'dot2 bound ms':>14s} {'of bound':>9s} "
          f"{'torch ms':>9s} {'x torch':>8s}")
    for r in rows:
        print(f"{r['format']:5s} {r['decimate']:3d} {r['ntaps']:4d} {r['seconds'] * 1e3:8.3f} {r['pairs_per_s'] / 1e9:9.2f} {r['gbytes_per_s']:8.1f} "
              f"{r['hbm_bound_s'] * 1e3:13.3f} {r['dot2_bound_s'] * 1e3:14.3f} {r['share_of_bound']:9.2f} {r['torch_seconds'] * 1e3:9.2f} "
              f"{r['speedup_over_torch']:8.1f}")
    rec = json.dumps({"tool": "ddc_probe", "device": torch.cuda.get_device_name(0), "rows": rows})
    print(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(rec + "\n")


if __name__ == "__main__":
    main()
