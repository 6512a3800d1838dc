#!/usr/bin/env python3
"""profiles/iq_norm_accuracy.json: the trained VT-CNN2 of tests/trained_vtcnn2.py on its held-out frames quantised to bytes at
a peak of 12, 50 and 120 LSB (+ a DC offset): accuracy at SNR >= 10 dB through predict_iq_u8(normalize="rms") and through the
plain scale = 1/127.5 path, per dtype, next to the f64 oracle's on the original float frames and on the reference-normalised
bytes (their difference is the quantisation margin tests/test_iq_norm_gpu.py allows, widened by the binomial 3 sigma).
A record, not a test: nothing is asserted here.  Needs the GPU (the net is trained on it).
    timeout -k 10 900 python tools/measure_iq_norm_accuracy.py [--out profiles/iq_norm_accuracy.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iq_norm_accuracy.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("no ROCm device: nothing is measured without the GPU")
    import test_iq_norm_gpu as G
    rec = G.accuracy_record()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
