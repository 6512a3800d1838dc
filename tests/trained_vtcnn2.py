"""Test infrastructure: a TRAINED canonical VT-CNN2 (T3, 11 classes) to hold the kernels to the f64 oracle on.

Every other T3 test runs on `synthetic_weights` -- the untrained glorot / he draws -- where the softmax is nearly uniform,
the conv2 filters are random (their sums are random walks) and the logits of all frames are alike.  A trained net differs
in exactly what the reduced-precision paths assume: matched conv2 filters (coherent sums: the fp8 feature scale),
decisive margins on most frames and thin ones on some, logits that vary from frame to frame.  No trained T3 weights
exist to bundle, and nothing trained is committed (2.83 M parameters), so the net is trained here, once per process:

  * the DeepSig recipe (RML2016.10a_VTCNN2_example.ipynb:229-260): Dropout 0.5 after conv1, conv2 and dense1, Adam at
    1e-3, categorical cross-entropy -- from `synthetic_weights(Topology.vtcnn2(11), seed=2016)`, the starting point of the
    untrained tests, on the 11-class frames of tests/signals.py (SNR 2 .. 18 dB), in batches of 256;
  * the frames enter training multiplied by INPUT_GAIN (about unit rms), and the exported conv1 kernel carries the gain
    instead (conv1 is linear ahead of its ReLU: the same function of the frames at their own 7.8e-3 level).  At that level
    itself Adam's first steps (1e-3 on every bias, the size of conv1's outputs) switch the ReLUs off and the loss stays at
    ln 11 for hundreds of steps;
  * torch autograd with the convolutions written as shifted slices + matmul (no convolution-algorithm search), every
    generator seeded and torch.use_deterministic_algorithms(True) while it runs: the same weights on every run of one
    device type;
  * exported in the layout VTCNN2.set_weights and oracle_np take: convs OIHW, denses (in, out), the channels-first
    Flatten index c * 132 + w.

    weights, stats = trained()                     # cached per process; on the GPU when there is one
    x, labels, snrs, ref = held_out()              # 4,096 frames of a seed training never saw + the f64 oracle on them
"""
import hashlib
import os
import time

import numpy as np

from modulationdetectioncnn_amd import Topology, synthetic_weights
from oracle import oracle_np as O
from signals import MODS11, modulated_frames11

TRAIN_SEED = 11          # frames the net is trained on
HELD_OUT_SEED = 2611     # frames the tests use (disjoint draws: another generator seed)
INIT_SEED = 2016         # synthetic_weights seed of the starting point
N_TRAIN = 1 << 16
EPOCHS = 4
BATCH = 256
INPUT_GAIN = 128.0       # a power of two: the fold into conv1 is exact in f32
LR = 1e-3
DROPOUT = 0.5
N_HELD_OUT = 4096

_cache = {}


def _torch():
    import torch
    return torch


def to_params(weights, device):
    """[(kernel, bias)] in the oracle's layouts -> the eight leaf tensors the training forward takes."""
    torch = _torch()
    return [torch.tensor(np.asarray(a, np.float32), device=device, requires_grad=True) for pair in weights for a in pair]


def export(params):
    """The leaf tensors -> [(kernel, bias)] float32 numpy in the oracle's layouts (the forward below keeps them in it)."""
    a = [p.detach().cpu().numpy().astype(np.float32) for p in params]
    return [(a[i], a[i + 1]) for i in range(0, 8, 2)]


def forward(params, x, train=False):
    """VT-CNN2 on x (n, 2, 128) -> logits (n, C), in the oracle's weight layouts; dropout when `train`.
    conv1 (1x3, 256) and conv2 (2x3 over 256 channels, 80) as shifted slices and one matmul each; the conv2 features are
    laid out (n, 80, 132) before the Flatten, so dense1's row index is c * 132 + w as in oracle_np.forward_vtcnn2."""
    torch = _torch()
    F = torch.nn.functional
    k1, b1, k2, b2, w1, bb1, w2, bb2 = params
    n = x.shape[0]
    xp = F.pad(x, (2, 2))                                                   # (n, 2, 132)
    a1 = torch.stack([xp[:, :, j:j + 130] for j in range(3)], dim=-1)       # (n, 2, 130, 3)
    y1 = torch.relu(a1 @ k1.reshape(256, 3).t() + b1)                        # (n, 2, 130, 256)  [h][w][c]
    y1 = F.dropout(y1, DROPOUT, train)
    y1p = F.pad(y1, (0, 0, 2, 2))                                           # (n, 2, 134, 256)
    win = torch.stack([y1p[:, :, j:j + 132, :] for j in range(3)], dim=-1)  # (n, h, w, c, j)
    a2 = win.permute(0, 2, 3, 1, 4).reshape(n * 132, 256 * 6)              # rows (n, w), columns (c, h, j)
    k2m = k2.permute(1, 2, 3, 0).reshape(256 * 6, 80)                       # OIHW -> rows (c, h, j)
    y2 = torch.relu(a2 @ k2m + b2).reshape(n, 132, 80)
    y2 = F.dropout(y2, DROPOUT, train)
    flat = y2.transpose(1, 2).reshape(n, 80 * 132)                           # channels-first Flatten: c * 132 + w
    d1 = F.dropout(torch.relu(flat @ w1 + bb1), DROPOUT, train)
    return d1 @ w2 + bb2


def fp8_feature_bound(weights, input_absmax=0.02):
    """numpy restatement of vtcnn2_fp8_pack's statistical conv2 bound (the comment above `kf`): per output channel
    |b2| + 12 x sqrt( sum_{c,h,j} w2^2 x (absmax^2 / 16 x sum_t k1[c][t]^2 + b1[c]^2) ), the largest over channels."""
    k1 = np.asarray(weights[0][0], np.float64).reshape(256, 3)
    b1 = np.asarray(weights[0][1], np.float64)
    k2 = np.asarray(weights[1][0], np.float64).reshape(80, 256, 6)
    b2 = np.asarray(weights[1][1], np.float64)
    c1ms = input_absmax ** 2 / 16.0 * (k1 ** 2).sum(axis=1) + b1 ** 2
    var = ((k2 ** 2).sum(axis=2) * c1ms[None, :]).sum(axis=1)
    return float((np.abs(b2) + 12.0 * np.sqrt(var)).max())


def fold_input_gain(weights, gain=INPUT_GAIN):
    """Weights trained on frames x `gain` -> the same net on the frames themselves: conv1's kernel x gain."""
    out = [(k.copy(), b.copy()) for k, b in weights]
    out[0] = ((out[0][0].astype(np.float64) * gain).astype(np.float32), out[0][1])
    return out


def checksum(weights):
    h = hashlib.sha256()
    for pair in weights:
        for a in pair:
            h.update(np.ascontiguousarray(a, np.float32).tobytes())
    return h.hexdigest()[:16]


def train(n_train=N_TRAIN, epochs=EPOCHS, batch=BATCH, device=None, steps=None, seed=TRAIN_SEED):
    """Train from the seed-2016 synthetic weights on frames x INPUT_GAIN; returns (weights with the gain folded into conv1,
    losses) -- `steps` stops early (the CPU test)."""
    torch = _torch()
    os.environ.setdefault("CUBLAS_WORKSPACE_CONFIG", ":4096:8")      # (read by the CUDA build's determinism check)
    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        torch.manual_seed(seed)                                      # dropout masks (every device's default generator)
        x, y, _ = modulated_frames11(n_train, seed=seed)
        xt = torch.from_numpy(x).to(device) * INPUT_GAIN
        yt = torch.from_numpy(y.astype(np.int64)).to(device)
        params = to_params(synthetic_weights(Topology.vtcnn2(11), seed=INIT_SEED), device)
        opt = torch.optim.Adam(params, lr=LR)
        order = np.random.default_rng(seed + 1)
        losses = []
        for _ in range(epochs):
            perm = torch.from_numpy(order.permutation(n_train)).to(device)
            for s in range(0, n_train - batch + 1, batch):
                idx = perm[s:s + batch]
                loss = torch.nn.functional.cross_entropy(forward(params, xt[idx], train=True), yt[idx])
                opt.zero_grad(set_to_none=True)
                loss.backward()
                opt.step()
                losses.append(float(loss.detach()))
                if steps is not None and len(losses) >= steps:
                    return fold_input_gain(export(params)), losses
        return fold_input_gain(export(params)), losses
    finally:
        torch.use_deterministic_algorithms(prev)


def held_out(n=N_HELD_OUT):
    """(x, labels, snrs, oracle) on frames of HELD_OUT_SEED, the f64 oracle (logits, probs, labels, flat, dense1) on the
    trained weights; cached."""
    key = ("held_out", n)
    if key not in _cache:
        w, _ = trained()
        x, lab, snr = modulated_frames11(n, seed=HELD_OUT_SEED)
        _cache[key] = (x, lab, snr, O.forward("vtcnn2", x, w, dtype=np.float64))
    return _cache[key]


def accuracy_by_snr(labels_true, labels_pred, snrs):
    return {int(s): float((labels_pred[snrs == s] == labels_true[snrs == s]).mean()) for s in np.unique(snrs)}


def trained():
    """(weights, stats), trained once per process.  stats: the oracle's held-out accuracy by SNR and at SNR >= 10 dB, the
    training wall time and device, the weights' checksum, the last epoch's mean loss, and the largest conv2 feature on the
    held-out frames over the fp8 statistical bound (fp8_feature_bound)."""
    if "net" not in _cache:
        torch = _torch()
        dev = "cuda" if torch.cuda.is_available() else "cpu"
        t0 = time.perf_counter()
        w, losses = train(device=dev)
        if dev == "cuda":
            torch.cuda.synchronize()
        secs = time.perf_counter() - t0
        _cache["net"] = (w, {"device": dev, "train_seconds": secs, "checksum": checksum(w), "steps": len(losses),
                             "loss_first_epoch": float(np.mean(losses[:N_TRAIN // BATCH])),
                             "loss_last_epoch": float(np.mean(losses[-(N_TRAIN // BATCH):]))})
        x, lab, snr, ref = held_out()
        st = _cache["net"][1]
        st["accuracy_by_snr"] = accuracy_by_snr(lab, ref["labels"], snr)
        st["accuracy_snr_ge_10"] = float((ref["labels"] == lab)[snr >= 10].mean())
        st["accuracy_all"] = float((ref["labels"] == lab).mean())
        bound = fp8_feature_bound(w)
        st["fp8_bound"] = bound
        st["max_feature"] = float(ref["flat"].max())
        st["max_feature_over_bound"] = float(ref["flat"].max()) / bound
        st["classes"] = list(MODS11)
    return _cache["net"]
