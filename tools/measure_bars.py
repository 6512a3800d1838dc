#!/usr/bin/env python3
"""ON THE GPU BOX: what the reduced-precision test bars are measured against.  Prints, per mode, the largest error
(relative to the largest |logit|, the unit of tests/test_vtcnn2_gpu.py's TOL) over the scenarios of the GPU tests, and the
label agreement with the f32 kernels on N(0, sigma) noise frames and on the signal-shaped frames of tests/signals.py.
The bars in the tests are about twice these maxima; re-run after touching a kernel's arithmetic.
--trained: only the trained-net scenario of tests/test_trained_vtcnn2_gpu.py (tests/trained_vtcnn2.py trains the net on the
GPU first) -> profiles/r06_measured_bars.json."""
import json, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from modulationdetectioncnn_amd import VTCNN2, Topology, synthetic_frames, synthetic_weights
from oracle import oracle_np as O            # checker
from signals import modulated_frames
from conftest import load_deployed_npz

out = {}
def model(classes, dtype, seed=2016, bias_scale=0.0, absmax=None):
    """dtype "fp8+bf16feat" = the fp8 mode with MDC_OPT_FP8_BF16_FEATURES (the pre-ABI-4 feature format)"""
    topo = Topology.vtcnn2(classes); w = synthetic_weights(topo, seed=seed, bias_scale=bias_scale)
    real = "fp8" if dtype.startswith("fp8") else dtype
    m = VTCNN2(topo, dtype=real, fp8_input_absmax=absmax if real == "fp8" else None, fp8_bf16_features=dtype == "fp8+bf16feat")
    m.set_weights(w); return m, w

xsig, _, _ = modulated_frames(1 << 16, seed=2016)
def progress(msg):      # (a hang is silent for minutes: say where we are, on stderr)
    print("[measure_bars]", msg, file=sys.stderr, flush=True)


def pcts(v):
    return [float(np.percentile(v, 50)), float(np.percentile(v, 99)), float(np.max(v))]


def trained_scenario():
    """The trained VT-CNN2 (tests/trained_vtcnn2.py) on its 4,096 held-out frames against the f64 oracle, and the label
    floors / per-SNR accuracy on 2^16 further frames against the f32 kernels."""
    import trained_vtcnn2 as T
    from signals import modulated_frames11
    progress("training")
    w, st = T.trained()
    x, lab, snr, ref = T.held_out()
    rl = ref["logits"]; scale = float(np.abs(rl).max()); own = np.abs(rl).max(axis=1)
    srt = np.sort(rl, axis=1); margin = (srt[:, -1] - srt[:, -2]) / own
    res = {"training": st, "held-out frames": len(x), "oracle: per-frame top-2 margin / own max|logit| p1 / p50": [float(np.percentile(margin, 1)), float(np.percentile(margin, 50))],
           "oracle: own max|logit| / batch max|logit| p1 / p50": [float(np.percentile(own / scale, 1)), float(np.percentile(own / scale, 50))]}
    bound = T.fp8_feature_bound(w); kf = int(np.floor(np.log2(224.0 / bound))); clip = 448.0 * 2.0 ** -kf
    res["fp8 occupancy"] = {"statistical bound": bound, "kf": kf, "clip level": clip, "largest feature": float(ref["flat"].max()),
                            "largest feature / bound": float(ref["flat"].max()) / bound,
                            "oracle features beyond the clip level": int((ref["flat"] > clip).sum())}
    xf, labf, snrf = modulated_frames11(1 << 16, seed=T.HELD_OUT_SEED + 1)
    xf = torch.from_numpy(xf).cuda()
    models = {}
    for mode in ("f32", "bf16", "fp8", "fp8+bf16feat"):
        progress("trained " + mode)
        m = VTCNN2(Topology.vtcnn2(11), dtype="fp8" if mode.startswith("fp8") else mode, fp8_bf16_features=mode == "fp8+bf16feat")
        m.set_weights(w); models[mode] = m
        lg = m.predict(x, tap="dense"); err = np.abs(lg - rl).max(axis=1)
        r = {"per-frame logit err / own max|logit| p50 / p99 / max": pcts(err / own),
             "logit err / batch max|logit| p50 / p99 / max": pcts(err / scale),
             "probs err / batch max|logit| max": float(np.abs(m.predict(x) - ref["probs"]).max() / scale),
             "small batches (1, 17, 257): logit err / their max|logit|": [float(np.abs(m.predict(x[:n], tap="dense") - rl[:n]).max() / np.abs(rl[:n]).max()) for n in (1, 17, 257)],
             "label agreement with the oracle (4,096)": float((m.predict_classes(x) == ref["labels"]).mean())}
        flat = m.predict(x, tap="flat")
        r["taps: flat / max (256 frames)"] = float(np.abs(flat[:256] - ref["flat"][:256]).max() / ref["flat"][:256].max())
        r["taps: hidden / max (256 frames)"] = float(np.abs(m.predict(x[:256], tap="hidden") - ref["dense1"][:256]).max() / np.abs(ref["dense1"][:256]).max())
        r["flat tap: largest value / oracle's largest"] = float(flat.max()) / float(ref["flat"].max())
        if mode == "fp8":
            res["fp8 occupancy"]["fp8 flat values at the clip level"] = int((flat >= clip).sum())
        res[mode] = r
    lf = models["f32"].predict_classes(xf)
    acc_f = models["f32"].accuracy_by_snr(xf, labf, snrf)[0]
    res["f32"]["accuracy by SNR (2^16 frames)"] = acc_f
    mc = VTCNN2(Topology.vtcnn2(11), dtype="fp8"); mc.set_weights(w)
    res["fp8"]["calibrated feature absmax"] = mc.calibrate_fp8_features(modulated_frames11(256, seed=T.HELD_OUT_SEED + 2)[0])
    models["fp8 calibrated"] = mc; res["fp8 calibrated"] = {}
    for mode in ("bf16", "fp8", "fp8+bf16feat", "fp8 calibrated"):
        m = models[mode]
        res[mode]["label agreement with the f32 kernels (2^16)"] = float((m.predict_classes(xf) == lf).float().mean())
        acc = m.accuracy_by_snr(xf, labf, snrf)[0]
        res[mode]["accuracy by SNR: largest |difference| from the f32 kernels'"] = max(abs(acc[s] - acc_f[s]) for s in acc)
    return res


if "--trained" in sys.argv:
    print(json.dumps(trained_scenario(), indent=1))
    sys.exit(0)

for dtype in ("bf16", "fp8", "fp8+bf16feat"):
    progress("vtcnn2 " + dtype)
    r = {}
    worst = 0.0; worst_p = 0.0
    for classes in (3, 11):
        m, w = model(classes, dtype)
        for n in (1, 16, 17, 64, 100, 257):
            x = synthetic_frames(n, seed=2016)
            ref = O.forward("vtcnn2", x, w, dtype=np.float64); scale = np.abs(ref["logits"]).max()
            worst = max(worst, float(np.abs(m.predict(x, tap="dense") - ref["logits"]).max() / scale))
            worst_p = max(worst_p, float(np.abs(m.predict(x) - ref["probs"]).max() / scale))
    r["parity: logits / max|logit|"] = worst; r["parity: probs / max|logit|"] = worst_p
    x = synthetic_frames(96, seed=7, sigma=0.5)
    m, w = model(11, dtype, seed=5, bias_scale=0.05, absmax=float(np.abs(x).max()))
    ref = O.forward("vtcnn2", x, w, dtype=np.float64); scale = np.abs(ref["logits"]).max()
    r["biases + large inputs: logits"] = float(np.abs(m.predict(x, tap="dense") - ref["logits"]).max() / scale)
    r["biases + large inputs: probs"] = float(np.abs(m.predict(x) - ref["probs"]).max() / scale)
    x = synthetic_frames(40, seed=3, sigma=0.1)
    m, w = model(11, dtype, seed=5, bias_scale=0.05, absmax=float(np.abs(x).max()))
    ref = O.forward("vtcnn2", x, w, dtype=np.float64, taps=True)
    r["taps: flat / max"] = float(np.abs(m.predict(x, tap="flat") - ref["flat"]).max() / np.abs(ref["flat"]).max())
    r["taps: hidden / max"] = float(np.abs(m.predict(x, tap="hidden") - ref["dense1"]).max() / np.abs(ref["dense1"]).max())
    mf, _ = model(11, "f32"); m, w = model(11, dtype)
    xa = synthetic_frames(8200, seed=21, device="cuda"); ra = mf.predict(xa, tap="dense"); scale = float(ra.abs().max())
    r["ragged vs f32 kernels: logits"] = max(float((m.predict(xa[:n].contiguous(), tap="dense") - ra[:n]).abs().max()) / scale
                                             for n in list(range(1, 49)) + [255, 256, 257, 511, 513, 4095, 4096, 4097, 4113, 8200])
    # signal-shaped frames against the f64 oracle (96 of them) and label agreement with the f32 kernels
    xs = xsig[:96]; ref = O.forward("vtcnn2", xs, w, dtype=np.float64); scale = np.abs(ref["logits"]).max()
    r["signal frames: logits"] = float(np.abs(m.predict(xs, tap="dense") - ref["logits"]).max() / scale)
    r["signal frames: probs"] = float(np.abs(m.predict(xs) - ref["probs"]).max() / scale)
    for classes in (11, 3):
        mf, _ = model(classes, "f32"); m, _ = model(classes, dtype)
        for tag, x in (("noise", synthetic_frames(1 << 16, seed=2016, device="cuda")), ("signal", torch.from_numpy(xsig).cuda())):
            r[f"label agreement C={classes} {tag}"] = float((mf.predict_classes(x) == m.predict_classes(x)).float().mean())
    # round 5: the error DISTRIBUTION and oracle-referenced label agreement on 4,096 frames of each kind
    # (f64 oracle), so that a maximum next to a bar can be read as a tail; a low-amplitude case (sigma 1e-3, a fifth of the
    # usual, the stated fp8 input range unchanged) -- what ADVICE r4 asked of the E4M3 feature scale
    for classes in (11, 3):
        progress(f"vtcnn2 {dtype}: oracle-referenced distributions, C = {classes}")
        m, w = model(classes, dtype)
        for tag, x in (("noise 5e-3", synthetic_frames(4096, seed=99)), ("signal", xsig[-4096:]), ("noise 1e-3", synthetic_frames(4096, seed=98, sigma=1e-3))):
            ref = O.forward("vtcnn2", x, w, dtype=np.float64)
            scale = np.abs(ref["logits"]).max()
            err = np.abs(m.predict(x, tap="dense") - ref["logits"]).max(axis=1) / scale      # per frame
            r[f"oracle C={classes} {tag}: logit err p50 / p99 / max"] = [float(np.percentile(err, 50)), float(np.percentile(err, 99)), float(err.max())]
            r[f"oracle C={classes} {tag}: label agreement"] = float((m.predict_classes(x) == ref["labels"]).mean())
            if classes == 11:      # the conv2 features themselves (the oracle's Flatten output against the flat tap)
                flat = m.predict(x[:512], tap="flat"); tru = ref["flat"][:512]
                pos = tru > 0
                r[f"features {tag}: flushed to zero (of the non-zero ones)"] = float(((flat == 0) & pos).sum() / pos.sum())
                rel = np.abs(flat - tru)[pos] / tru[pos]
                r[f"features {tag}: relative error p50 / p99"] = [float(np.percentile(rel, 50)), float(np.percentile(rel, 99))]
                r[f"features {tag}: largest / rms of the non-zero"] = [float(tru.max()), float(np.sqrt((tru[pos] ** 2).mean()))]
    out["vtcnn2 " + dtype] = r
g = os.path.join(ROOT, "tests", "golden", "weights")
for name in ("3convmodrecnets_CNN2_0.5", "convmodrecnets_CNN2_0.5", "5convmodrecnets_CNN2_0.5"):
    progress("deployed " + name)
    flat = [a for p in load_deployed_npz(name) for a in p]
    mf = VTCNN2.from_npz(os.path.join(g, name + ".npz"))
    ref = O.forward_deployed(xsig, *flat, dtype=np.float64)
    d = ref["dense"]; srt = np.sort(d, axis=1); scale = max(1.0, float(np.abs(d).max()))
    decided = (srt[:, -1] - srt[:, -2]) > 1e-5 * scale
    pf = mf.predict(xsig); lf = mf.predict_classes(xsig)
    r = {"f32 signal: probs err": float(np.abs(pf - ref["probs"]).max()), "f32 signal: decided fraction": float(decided.mean()),
         "f32 signal: label mismatches among decided": int((lf[decided] != ref["labels"][decided]).sum()),
         "f32 signal: label mismatches all": int((lf != ref["labels"]).sum()),
         "f32 signal: dense err / scale": float(np.abs(mf.predict(xsig, tap="dense") - d).max() / scale)}
    for dtype in ("bf16", "f16", "fp8"):
        m = VTCNN2.from_npz(os.path.join(g, name + ".npz"), dtype=dtype)
        r[f"{dtype} signal: probs err vs f64"] = float(np.abs(m.predict(xsig) - ref["probs"]).max())
        for tag, x in (("noise 5e-3", synthetic_frames(1 << 16, seed=77, sigma=5e-3, device="cuda")),
                       ("noise 0.1", synthetic_frames(1 << 16, seed=77, sigma=0.1, device="cuda")), ("signal", torch.from_numpy(xsig).cuda())):
            r[f"{dtype} label agreement {tag}"] = float((mf.predict_classes(x) == m.predict_classes(x)).float().mean())
    out["deployed " + name] = r
print(json.dumps(out, indent=1))
