#!/usr/bin/env python3
"""An SDR capture (interleaved I,Q samples: unsigned bytes of an RTL-SDR -- the front-end of the reference's README.md:5 --,
signed bytes of a HackRF, or signed 16-bit little-endian samples of a USRP / SDRplay / bladeRF / Airspy) -> one label per
window, whatever the gain and DC offset of the capture: each window is brought to the level the nets were trained at
(predict_iq(normalize="rms")), and windows whose power lies below the squelch get label -1.

    python examples/classify_capture.py capture.bin --weights tests/golden/weights/convmodrecnets_CNN2_0.5.npz --hop 64 --squelch -35
Without a capture file it classifies a synthetic one: bursts of tones at three gains with silence between them."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from modulationdetectioncnn_amd import VTCNN2      # noqa: E402


DTYPES = {"cu8": np.uint8, "ci8": np.int8, "ci16": "<i2"}


def synthetic_capture(fmt="cu8", seed=1):
    rng = np.random.default_rng(seed)
    parts = []
    for gain in (4.0, 30.0, 110.0):
        t = np.arange(128 * 40)
        burst = gain * np.exp(2j * np.pi * (0.07 * t + rng.uniform()))
        quiet = np.zeros(128 * 20, complex)
        z = np.concatenate([burst, quiet]) + 0.4 * (rng.standard_normal(128 * 60) + 1j * rng.standard_normal(128 * 60))
        parts.append(z)
    z = np.concatenate(parts)
    if fmt == "cu8":
        iq = np.stack([z.real + 129.3, z.imag + 126.1], axis=1)      # a tuner's DC offset: the midpoint is not 127.5
        return np.clip(np.rint(iq), 0, 255).astype(np.uint8).reshape(-1)
    k = 1.0 if fmt == "ci8" else 256.0                                 # the same signal in the wider format's LSBs
    iq = np.stack([k * (z.real + 1.8), k * (z.imag - 1.4)], axis=1)
    lo, hi = (-128, 127) if fmt == "ci8" else (-32768, 32767)
    return np.clip(np.rint(iq), lo, hi).astype(DTYPES[fmt]).reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("capture", nargs="?", help="file of interleaved samples I0 Q0 I1 Q1 ... in --format")
    ap.add_argument("--format", choices=["cu8", "ci8", "ci16"], default="cu8",
                    help="sample format: unsigned bytes (RTL-SDR), signed bytes (HackRF), signed 16-bit little-endian (USRP sc16, ...)")
    ap.add_argument("--weights", default=None, help=".h5 / .npz of a deployed net (default: synthetic weights)")
    ap.add_argument("--hop", type=int, default=128, help="sample pairs between windows (128: disjoint frames)")
    ap.add_argument("--level", type=float, default=7.8e-3, help="complex rms every window is normalised to")
    ap.add_argument("--squelch", type=float, default=-35.0, help="dBFS below which a window gets label -1")
    a = ap.parse_args()
    iq = np.fromfile(a.capture, DTYPES[a.format]) if a.capture else synthetic_capture(a.format)
    iq = iq[:iq.size // 256 * 256] if a.hop == 128 else iq[:iq.size // 2 * 2]
    if a.weights is None:
        model = VTCNN2.synthetic("deployed3")
    else:
        model = VTCNN2.from_npz(a.weights) if a.weights.endswith(".npz") else VTCNN2.from_h5(a.weights)
    probs, labels, dbfs = model.predict_iq(iq, a.format, hop=a.hop, normalize="rms", level=a.level, squelch_dbfs=a.squelch, return_power=True)
    print(f"{labels.size} windows, {int((labels < 0).sum())} below {a.squelch} dBFS")
    for k in np.unique(labels):
        sel = labels == k
        print(f"  label {int(k):2d}: {int(sel.sum()):6d} windows, power {dbfs[sel].min():7.1f} .. {dbfs[sel].max():6.1f} dBFS")


if __name__ == "__main__":
    main()
