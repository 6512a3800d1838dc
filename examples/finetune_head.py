#!/usr/bin/env python3
"""Adapt a VT-CNN2 to a channel by fine-tuning its dense layers on the MI355X (VTCNN2.fit_head: dense1 10560 x 256 and dense2
256 x C, 2,706,443 of the net's 2,830,427 parameters, with the two conv layers frozen -- transfer learning).

Takes a VT-CNN2 (--weights FILE: a Keras .h5 whose classes are RML2016.10a's eleven modulations in order; else a synthetic
initialisation), builds a labelled data set with the library's own generator (synth_recipe / synth_dataset; --fading sends every
frame through synth_fading's Rician multipath channel), and prints the accuracy by SNR on held-out frames before and after the
fit.  The features are computed once, through the model's own engine at --dtype, so the head is tuned on what the deployed
precision delivers.

    python examples/finetune_head.py [--weights FILE] [--dtype f32|bf16|fp8] [--frames 32768] [--val-frames 8192] [--fading]
                                     [--snrs 0,6,12,18] [--epochs 10] [--batch-size 1024] [--lr 1e-3] [--dropout 0.5] [--seed 2016]
                                     [--save FILE]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from modulationdetectioncnn_amd import VTCNN2, Topology, frontend      # noqa: E402


def by_snr(model, X, labels, snr_db):
    acc = {}
    pred = model.predict_classes(X).cpu().numpy()
    for s in sorted(set(snr_db.tolist())):
        sel = snr_db == s
        acc[int(s)] = float((pred[sel] == labels[sel]).mean())
    return acc


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--weights")
    ap.add_argument("--dtype", default="f32", choices=("f32", "bf16", "fp8"))
    ap.add_argument("--frames", type=int, default=1 << 15)
    ap.add_argument("--val-frames", type=int, default=1 << 13)
    ap.add_argument("--fading", action="store_true")
    ap.add_argument("--snrs", default="0,6,12,18")
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--batch-size", type=int, default=1024)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--dropout", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=2016)
    ap.add_argument("--save", help="write the fine-tuned model as a Keras .h5")
    a = ap.parse_args(argv)
    recipe = frontend.synth_recipe(snrs_db=[int(s) for s in a.snrs.split(",")], fading=frontend.synth_fading() if a.fading else None)
    if a.weights:
        model = VTCNN2.from_h5(a.weights, dtype=a.dtype)
    else:
        model = VTCNN2.synthetic(Topology.vtcnn2(len(recipe.mods)), seed=a.seed, dtype=a.dtype)
    X, labels, _snr = frontend.synth_dataset(a.frames, recipe, seed=a.seed)
    Xv, lv, sv = frontend.synth_dataset(a.val_frames, recipe, seed=a.seed, first_frame=a.frames)
    lv_h, sv_h = lv.cpu().numpy(), sv.cpu().numpy()
    before = by_snr(model, Xv, lv_h, sv_h)
    hist = model.fit_head(X, labels, batch_size=a.batch_size, epochs=a.epochs, validation_data=(Xv, lv), dropout=(a.dropout, a.dropout),
                          lr=a.lr, seed=a.seed, dropout_seed=a.seed, patience=None, verbose=1)
    after = by_snr(model, Xv, lv_h, sv_h)
    print(f"{'SNR dB':>7s} {'before':>8s} {'after':>8s}      ({a.val_frames} held-out frames, {len(recipe.mods)} classes, dtype {a.dtype}"
          f"{', faded' if a.fading else ''})")
    for s in before:
        print(f"{s:7d} {before[s]:8.3f} {after[s]:8.3f}")
    print(f"val_loss {hist.history['val_loss'][0]:.4f} -> {hist.history['val_loss'][-1]:.4f}, val_accuracy {hist.history['val_accuracy'][-1]:.3f}")
    if a.save:
        model.save(a.save)
    model._release()
    return before, after


if __name__ == "__main__":
    main()
