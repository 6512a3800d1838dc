#!/usr/bin/env python3
"""Time of one head-training step (csrc/head_train.hip: VT-CNN2's head, 10560 -> 256 -> 11, Dropout (0.5, 0.5), Adam applied) at
batches 256 / 1,024 / 8,192, next to a torch-ROCm statement of the SAME step in the same process: torch.matmul and elementwise
ops on the same rows, the same Dropout masks (made once, outside the timed region: the torch side is not charged for the
generator), Keras' clipped cross-entropy with its hand-written backward, and a hand-written Adam of TensorFlow 2.4's form.  The
torch statement is the yardstick, not an earlier build.

Also: the share of the f32 MFMA peak on the two big products (Z1 = A W1 and dW1 = A^T dZ1: 2 x 2 x batch x 10560 x 256 FLOP; peak
157.3 TFLOP/s = 256 CUs x 4 SIMDs x 64 FLOP/clk x 2.4 GHz), charged with the WHOLE step's time -- a lower bound of what the two
GEMM kernels themselves reach --, and the step's five kernels one by one (device events around each launch are not available
through the C ABI, so the split is taken with apply = 0 / evaluation runs: evaluation = launches 1, 2 and the statistics).

Timing: device events around `reps` back-to-back steps after a warm-up, the median of `rounds` windows, the two sides
alternating within every round; `spread` = (max - min) / median of a side's windows.  Needs the GPU; prints a table and one JSON
line.

    python tools/head_train_probe.py [--batches 256 1024 8192] [--rounds 7] [--reps 20] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, H, C = 10560, 256, 11
PEAK_F32_MFMA = 256 * 4 * 64 * 2.4e9


def _window(fn, reps, torch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def dropout_scale(torch, rate, seed, step, n, nelem, site):
    """include/mdc.h's generator (mdc_trainer_set_dropout) in torch int64 arithmetic, masked to 32 bits: (n, nelem) of 0 or 1 / (1 - rate)."""
    M = 0xFFFFFFFF

    def fmix32(h):
        h = h ^ (h >> 16)
        h = (h * 0x85EBCA6B) & M
        h = h ^ (h >> 13)
        h = (h * 0xC2B2AE35) & M
        return h ^ (h >> 16)

    k_step = fmix32(torch.tensor([(seed + 0x9E3779B9 * (step + 1)) & M], dtype=torch.int64, device="cuda"))
    frames = torch.arange(n, dtype=torch.int64, device="cuda")
    k_frame = fmix32(k_step ^ ((frames * 0x85EBCA6B + site) & M))
    u = fmix32((k_frame[:, None] + torch.arange(nelem, dtype=torch.int64, device="cuda")[None, :] * 0xC2B2AE35) & M)
    thr = int(np.floor(float(np.float32(rate)) * 4294967296.0))
    return (u >= thr).float() * float(np.float32(1) / (np.float32(1) - np.float32(rate)))


class TorchStep:
    """The step as torch-ROCm states it: matmuls and elementwise ops, Keras' loss backward by hand, Adam by hand."""

    def __init__(self, w, s0, s1, torch, lr=1e-3, b1=0.9, b2=0.999, eps=1e-7):
        self.t = torch
        self.p = [torch.from_numpy(a.copy()).cuda() for pair in w for a in pair]
        self.m = [torch.zeros_like(a) for a in self.p]
        self.v = [torch.zeros_like(a) for a in self.p]
        self.s0, self.s1, self.it, self.hp = s0, s1, 0, (lr, b1, b2, eps)

    def __call__(self, f, y):
        t = self.t
        w1, bb1, w2, bb2 = self.p
        n = f.shape[0]
        a = f * self.s0
        z1 = t.addmm(bb1, a, w1)
        h = t.relu(z1) * self.s1
        p = t.softmax(t.addmm(bb2, h, w2), dim=1)
        s = p.sum(dim=1, keepdim=True)
        q = p / s
        qc = q.clamp(1e-7, 1 - 1e-7)
        loss = -(y * qc.log()).sum()
        gq = t.where((q >= 1e-7) & (q <= 1 - 1e-7), -y / qc, t.zeros_like(q))
        gp = (gq - (gq * q).sum(dim=1, keepdim=True)) / s
        dz2 = p * (gp - (gp * p).sum(dim=1, keepdim=True)) / n
        dz1 = (dz2 @ w2.t()) * self.s1 * (z1 > 0)
        grads = [a.t() @ dz1, dz1.sum(dim=0), h.t() @ dz2, dz2.sum(dim=0)]
        lr, b1, b2, eps = self.hp
        self.it += 1
        alpha = lr * (1 - b2 ** self.it) ** 0.5 / (1 - b1 ** self.it)
        for w, g, m, v in zip(self.p, grads, self.m, self.v):
            m.add_(g - m, alpha=1 - b1)
            v.add_(g * g - v, alpha=1 - b2)
            w.sub_(m * alpha / (v.sqrt() + eps))
        return loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 1024, 8192])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    a = ap.parse_args()
    import torch
    from modulationdetectioncnn_amd.training import HeadTrainer
    if not torch.cuda.is_available():
        raise SystemExit("head_train_probe needs the GPU: a CPU run says nothing about speed")
    rng = np.random.default_rng(0)
    l1, l2 = np.sqrt(6.0 / (K + H)), np.sqrt(6.0 / (H + C))
    w = [(rng.uniform(-l1, l1, (K, H)).astype(np.float32), np.zeros(H, np.float32)), (rng.uniform(-l2, l2, (H, C)).astype(np.float32), np.zeros(C, np.float32))]
    rec = {"tool": "head_train_probe", "device": torch.cuda.get_device_name(0), "K": K, "H": H, "C": C, "rounds": a.rounds, "reps": a.reps, "cases": []}
    print(f"{'batch':>6} {'hip step us':>12} {'spread':>7} {'torch step us':>14} {'spread':>7} {'torch/hip':>9} {'MFMA share':>10} {'grad only us':>13} {'eval us':>8}")
    for n in a.batches:
        f = torch.from_numpy((np.maximum(rng.standard_normal((n, K)), 0) * 0.05).astype(np.float32)).cuda()
        y = torch.nn.functional.one_hot(torch.from_numpy(rng.integers(0, C, n)), C).float().cuda()
        s0, s1 = dropout_scale(torch, 0.5, 1, 0, n, K, 0), dropout_scale(torch, 0.5, 1, 0, n, H, 1)      # step 0's masks, reused at every step
        tr = HeadTrainer(K, H, C, w, device=0, max_batch=n, dropout=(0.5, 0.5), dropout_seed=1)
        ts = TorchStep(w, s0, s1, torch)
        # the same first step on both sides (the same masks at iteration 0), before anything is timed
        tr.train_batch(f, y)
        ts(f, y)
        torch.cuda.synchronize()
        agree = max(float((torch.from_numpy(k).cuda() - p).abs().max()) for (k, p) in zip([t for pr in tr.get_weights() for t in pr], ts.p))
        sides = {"hip": lambda: tr.train_batch(f, y), "torch": lambda: ts(f, y), "hip_grad": lambda: tr.train_batch(f, y, apply=False),
                 "hip_eval": lambda: tr.evaluate_enqueue(f, y)}
        for fn in sides.values():
            _window(fn, 3, torch)
        wins = {k: [] for k in sides}
        for _ in range(a.rounds):
            for k, fn in sides.items():
                wins[k].append(_window(fn, a.reps, torch))
        tr.read()
        med = {k: float(np.median(v)) for k, v in wins.items()}
        spread = {k: float((max(v) - min(v)) / np.median(v)) for k, v in wins.items()}
        share = 4.0 * n * K * H / med["hip"] / PEAK_F32_MFMA
        print(f"{n:>6} {med['hip'] * 1e6:>12.1f} {spread['hip']:>7.3f} {med['torch'] * 1e6:>14.1f} {spread['torch']:>7.3f} {med['torch'] / med['hip']:>9.2f} "
              f"{share:>10.3f} {med['hip_grad'] * 1e6:>13.1f} {med['hip_eval'] * 1e6:>8.1f}")
        rec["cases"].append({"batch": n, "median_s": med, "spread": spread, "torch_over_hip": med["torch"] / med["hip"], "mfma_share_whole_step": share,
                             "first_step_max_weight_difference": agree})
        del tr, ts, f, y, s0, s1
        torch.cuda.empty_cache()
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
