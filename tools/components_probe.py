#!/usr/bin/env python3
"""Time of mdc_iq_spectrogram_components (connected components of a thresholded spectrogram, csrc/iq_components.hip) on the
device, next to scipy.ndimage.label on the host as the only available yardstick.

Reach (1, 1) -- scipy's 3 x 3 structure -- on (rows, nfft) in {(16384, 1024), (65536, 256), (4096, 4096)} float32 spectrograms and
three masks: "noise", a noise-only spectrogram (the mean of 8 exponential segments per cell) at frontend.detection_threshold's
6 dB over the flat floor; "hopper", the same noise with a hopper's dwells drawn onto it (boxes of nfft / 24 bins by rows / 64 rows,
14 dB over the floor, one after another at centres spread over the band, the test capture scaled up); "density 0.3", uniform
random cells.  Per shape and mask: milliseconds, components, and the share of the HBM floor -- one read of the matrix plus one
write and one read of the labels, 12 * rows * nfft bytes at the measured copy rate of the MI355X (6.29 TB/s).  The yardstick
labels the same mask (copied to the host, centred) with scipy.ndimage.label; the two labellings are compared up to renumbering
before anything is timed.

Timing: device events around `reps` back-to-back calls after a warm-up, the median of `rounds` such windows, one process.  Needs
the GPU; prints a table and one JSON line.

    python tools/components_probe.py [--rounds 5] [--reps 10] [--out profiles/components_probe.json] [--no-yardstick]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_COPY_BYTES_PER_S = 6.29e12
SHAPES = [(16384, 1024), (65536, 256), (4096, 4096)]
REACH = (1, 1)


def _time(fn, reps, torch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def _noise(rows, nfft, g, torch):
    spec = torch.zeros((rows, nfft), dtype=torch.float32, device="cuda")
    seg = torch.empty((rows, nfft), dtype=torch.float32, device="cuda")
    for _ in range(8):      # a row of the spectrogram averages 8 segments
        spec += seg.exponential_(1.0, generator=g)
    return spec * (1e-6 / 8)


def _masks(rows, nfft, g, torch, frontend):
    """name -> (spec, thresh) on the device"""
    noise = _noise(rows, nfft, g, torch)
    hopper = noise.clone()
    width, dwell = max(3, nfft // 24), max(3, rows // 64)
    for i, r0 in enumerate(range(dwell // 2, rows - dwell, dwell + max(1, dwell // 8))):
        c0 = (i * 7919) % (nfft - width)      # centres spread over the band, in centred columns
        cols = (torch.arange(c0, c0 + width, device="cuda") + nfft // 2) % nfft
        hopper[r0:r0 + dwell, cols] *= 25.0
    uniform = torch.rand((rows, nfft), dtype=torch.float32, device="cuda", generator=g)
    return {"noise": (noise, frontend.detection_threshold(noise)), "hopper": (hopper, frontend.detection_threshold(hopper)),
            "density 0.3": (uniform, torch.full((nfft,), 0.7, dtype=torch.float32, device="cuda"))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    ap.add_argument("--no-yardstick", action="store_true", help="skip scipy.ndimage.label (and with it the comparison of the results)")
    a = ap.parse_args()
    import torch
    from modulationdetectioncnn_amd import _cabi, frontend
    if not torch.cuda.is_available():
        raise SystemExit("components_probe needs the GPU: a CPU run says nothing about speed")
    ndimage = None
    if not a.no_yardstick:
        from scipy import ndimage
    L = _cabi.lib()
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(1)
    capacity = 1 << 16
    table = []
    for rows, nfft in SHAPES:
        labels = torch.empty((rows, nfft), dtype=torch.int32, device="cuda")
        comps = torch.empty((capacity, 4), dtype=torch.int64, device="cuda")
        count = torch.empty((1,), dtype=torch.int64, device="cuda")
        work = torch.empty((frontend.components_workspace(rows, nfft) // 8 + 2,), dtype=torch.int64, device="cuda")
        ws = work.data_ptr() + (-work.data_ptr()) % 16
        for name, (spec, thresh) in _masks(rows, nfft, g, torch, frontend).items():
            def ours():
                _cabi.check(L.mdc_iq_spectrogram_components(spec.data_ptr(), rows, nfft, thresh.data_ptr(), REACH[0], REACH[1], labels.data_ptr(),
                                                            comps.data_ptr(), capacity, count.data_ptr(), ws, stream))
            ours()
            ours()
            torch.cuda.synchronize()
            n = int(count.item())
            host_s = None
            if ndimage is not None:
                mask = np.roll((spec > thresh[None, :]).cpu().numpy(), nfft // 2, axis=1)
                t0 = time.perf_counter()
                theirs, m = ndimage.label(mask, structure=np.ones((3, 3), int))
                host_s = time.perf_counter() - t0
                mine = np.roll(labels.cpu().numpy(), nfft // 2, axis=1)
                on = mask.reshape(-1)
                pairs = np.unique(mine.reshape(-1)[on].astype(np.int64) * (m + 1) + theirs.reshape(-1)[on])
                if not (m == n == pairs.size and (mine.reshape(-1)[~on] == -1).all()):
                    raise SystemExit(f"({rows}, {nfft}) {name}: the kernels ({n} components) and scipy.ndimage.label ({m}) disagree")
                del mask, theirs, mine, on, pairs
            t = [_time(ours, a.reps, torch) for _ in range(a.rounds)]
            sec = float(np.median(t))
            floor = 12.0 * rows * nfft / HBM_COPY_BYTES_PER_S
            table.append(dict(rows=rows, nfft=nfft, mask=name, on_share=float((spec > thresh[None, :]).float().mean()), components=n, seconds=sec,
                              seconds_min=float(min(t)), hbm_floor_s=floor, share_of_hbm_floor=floor / sec, scipy_label_seconds=host_s,
                              speedup_over_scipy=None if host_s is None else host_s / sec))
        del labels, comps, count, work
        torch.cuda.empty_cache()
    print(f"device: {torch.cuda.get_device_name(0)}; reach {REACH}; median of {a.rounds} windows of {a.reps} calls")
    print(f"{'rows':>7s} {'nfft':>5s} {'mask':>12s} {'on':>6s} {'components':>11s} {'ms':>8s} {'HBM floor ms':>13s} {'of floor':>9s} {'scipy ms':>9s} {'x scipy':>8s}")
    for r in table:
        host = ("        -        -" if r["scipy_label_seconds"] is None else f"{r['scipy_label_seconds'] * 1e3:9.1f} {r['speedup_over_scipy']:8.0f}")
        print(f"{r['rows']:7d} {r['nfft']:5d} {r['mask']:>12s} {r['on_share']:6.3f} {r['components']:11d} {r['seconds'] * 1e3:8.3f} "
              f"{r['hbm_floor_s'] * 1e3:13.4f} {r['share_of_hbm_floor']:9.3f} {host}")
    rec = json.dumps({"tool": "components_probe", "device": torch.cuda.get_device_name(0), "reach": list(REACH), "rows": table})
    print(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(rec + "\n")


if __name__ == "__main__":
    main()
