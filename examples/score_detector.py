#!/usr/bin/env python3
"""How often is "what transmitted when, where, and what modulation" right?  Design a scene of emitters, synthesise it on the device
with its truth table (frontend.synth_scene / synth_capture / scene_truth: mdc_iq_synth_capture), run the detector over the capture
(VTCNN2.detect_iq, or scan_iq with --scan) and score its records against the truth (frontend.score_detections): dwells found and
missed, false detections, and the label confusion over the found ones.

The scene is the built-in default -- a continuous QPSK, a bursty BPSK, a GFSK hopper over four carriers and two emitters that share
bins at different times -- or one emitter per --emitter flag:

    --emitter MOD,SPS,CENTRE[/CENTRE...],LEVEL_DB[,START,ON,PERIOD]      e.g.  --emitter GFSK,32,0.05/0.15/0.25,20,16384,49152,65536

(samples per symbol and the schedule in capture samples; several centres make a hopper).  Weights come from --weights (a Keras
.h5 file whose classes are the recipe's modulations in order), or from a short fit on synth_dataset of the same recipe.
--net vtcnn2 classifies with the canonical VT-CNN2 instead of cnn.py's small net: its dense head is fitted to the recipe's classes
with VTCNN2.fit_head for --head-epochs epochs (the conv layers stay as --weights or the synthetic initialisation gives them).

    python examples/score_detector.py [--pairs 524288] [--noise-rms 300] [--seed 2016] [--emitter ...] [--weights FILE] [--epochs 3] [--scan]
                                      [--net cnnpy|vtcnn2] [--head-epochs 3]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from modulationdetectioncnn_amd import VTCNN2, Topology, frontend      # noqa: E402

MODS = ("QPSK", "BPSK", "GFSK", "8PSK")
NFFT, AVG = 1024, 8


def default_emitters():
    row = NFFT // 2 * AVG
    return [dict(mod="QPSK", samples_per_symbol=32, centre=-0.35, level_db=20.0),
            dict(mod="BPSK", samples_per_symbol=32, centre=-0.15, level_db=20.0, start=10 * row, on=20 * row, period=40 * row),
            dict(mod="GFSK", samples_per_symbol=32, centre=[0.05, 0.15, 0.25, 0.35], level_db=20.0, start=4 * row, on=12 * row, period=16 * row),
            dict(mod="8PSK", samples_per_symbol=32, centre=0.45, level_db=20.0, start=8 * row, on=24 * row),
            dict(mod="QPSK", samples_per_symbol=32, centre=0.45, level_db=20.0, start=60 * row, on=30 * row)]


def parse_emitter(text):
    f = text.split(",")
    if len(f) not in (4, 7):
        raise SystemExit(f"--emitter {text!r}: MOD,SPS,CENTRE[/CENTRE...],LEVEL_DB[,START,ON,PERIOD]")
    centres = [float(c) for c in f[2].split("/")]
    em = dict(mod=f[0], samples_per_symbol=float(f[1]), centre=centres if len(centres) > 1 else centres[0], level_db=float(f[3]))
    if len(f) == 7:
        em.update(start=float(f[4]), on=float(f[5]), period=float(f[6]))
    return em


def head_tuned_vtcnn2(recipe, args):
    """The canonical VT-CNN2 with its dense head fitted to the recipe's classes (VTCNN2.fit_head; the conv layers are frozen)."""
    if args.weights:
        model = VTCNN2.from_h5(args.weights)
    else:
        model = VTCNN2.synthetic(Topology.vtcnn2(len(recipe.mods)), seed=args.seed)
    if args.head_epochs <= 0:
        return model
    frames = min(args.frames, 1 << 14)      # 2^14 rows of 10,560 features: 0.7 GB
    X, labels, _ = frontend.synth_dataset(frames, recipe, seed=args.seed + 1)
    out = model.fit_head(X, labels, batch_size=1024, epochs=args.head_epochs, classes=len(recipe.mods), seed=args.seed, patience=None)
    return out if isinstance(out, VTCNN2) else model


def trained_model(recipe, args):
    from modulationdetectioncnn_amd.training import to_onehot
    if args.net == "vtcnn2":
        return head_tuned_vtcnn2(recipe, args)
    topo = Topology.cnnpy(10, 10, len(recipe.mods))      # cnn.py's net: the trainer takes any number of classes for it
    model = VTCNN2.synthetic(topo, seed=args.seed)
    if args.weights:
        model.load_weights(args.weights)
        return model
    X, labels, _ = frontend.synth_dataset(args.frames, recipe, seed=args.seed + 1)
    Y = to_onehot(labels.cpu().numpy(), len(recipe.mods))
    model.compile(loss="categorical_crossentropy", optimizer="adam", lr=1e-3)
    model.fit(X, Y, batch_size=1024, epochs=args.epochs, verbose=0, seed=args.seed)
    return model


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1 << 19)
    ap.add_argument("--noise-rms", type=float, default=300.0)
    ap.add_argument("--seed", type=int, default=2016)
    ap.add_argument("--emitter", action="append", default=[])
    ap.add_argument("--weights")
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--frames", type=int, default=1 << 15, help="frames of the short fit")
    ap.add_argument("--min-overlap", type=float, default=0.5)
    ap.add_argument("--net", choices=("cnnpy", "vtcnn2"), default="cnnpy", help="the classifier: cnn.py's small net (fit) or VT-CNN2 (fit_head)")
    ap.add_argument("--head-epochs", type=int, default=3, help="--net vtcnn2: epochs of the head fit (0: classify with the weights as they are)")
    ap.add_argument("--scan", action="store_true", help="score scan_iq's emitters (one record per emitter, no time axis) instead of detect_iq's")
    ap.add_argument("--floor", choices=("flat", "per-bin", "cfar"), default="flat",
                    help="detect_iq's noise floor: one level, every bin's median over time, or a local order-statistic floor per cell")
    args = ap.parse_args(argv)
    emitters = [parse_emitter(t) for t in args.emitter] or default_emitters()
    mods = tuple(dict.fromkeys(list(MODS) + [e["mod"] for e in emitters]))
    recipe = frontend.synth_recipe(mods=mods, snrs_db=(0, 6, 12, 18))
    scene = frontend.synth_scene(recipe, emitters, args.noise_rms)
    iq, saturated = frontend.synth_capture(args.pairs, scene, seed=args.seed, return_saturated=True)
    truth = frontend.scene_truth(scene, args.pairs, args.seed)
    model = trained_model(recipe, args)
    if args.scan:
        records = [dict(r, first_pair=0, stop_pair=args.pairs) for r in model.scan_iq(iq, "ci16", nfft=NFFT, avg=AVG)]
    else:
        records = model.detect_iq(iq, "ci16", nfft=NFFT, avg=AVG, floor=args.floor, batched=True)
    score = frontend.score_detections(records, truth, min_overlap=args.min_overlap, classes=len(mods))
    hit = dict(score["found"])
    print(f"{args.pairs} pairs, {len(scene.emitters)} emitters, {saturated} clamped components; {len(truth)} truth dwells, {len(records)} detections")
    print(f"{'emitter':>7s} {'mod':6s} {'dwell':>5s} {'first_pair':>10s} {'stop_pair':>10s} {'centre':>8s} {'level dB':>8s}  found as")
    for t, row in enumerate(truth):
        d = hit.get(t)
        as_ = "-- missed --" if d is None else f"detection {d}: centre {records[d]['centre']:+.4f}, label {mods[records[d]['label']] if records[d]['label'] >= 0 else '-'}"
        print(f"{row['emitter']:7d} {row['mod']:6s} {row['dwell']:5d} {row['first_pair']:10d} {row['stop_pair']:10d} {row['centre']:+8.4f} {row['level_db']:8.1f}  {as_}")
    print(f"found {len(score['found'])} of {len(truth)}, missed {len(score['missed'])}, false detections {len(score['false'])}; "
          f"label accuracy over the found ones {score['accuracy']:.3f}")
    print("confusion (rows: truth, columns: detected):", ", ".join(mods))
    print(score["confusion"])
    model._release()
    return score


if __name__ == "__main__":
    main()
