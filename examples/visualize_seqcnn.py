#!/usr/bin/env python3
"""kgcn visualize --config config_cnn.pos.json --ig_label_target 1 (sample_protein/sequence/03run.sh, its second step) on the MI355X
path: integrated gradients of the protein-sequence CNN (cnn.py:SeqCNN, models.SeqCNN) with respect to its embedded layer, through
visualization.seqcnn_integrated_gradients.  config_cnn.pos.json reads pos_dataset.jbl, the positive proteins alone, numbered in
their own order; --proteins positives (the default) selects them from the dataset the same way, --proteins all takes every
sequence.  Loads parameters examples/train_seqcnn.py saved (--params, its --save PATH), or does a short fit itself (--epochs).
Writes one {header}_{id:04d}_task_0_{assay}_embedded_layer_scaling.jbl per protein (joblib, the keys kgcn/visualization.py dumps:
embedded_layer, embedded_layer_IG [L, E], amino_acid_seq, ...; 04result_list.py collects them by that name) and logs the prediction
score, check score (end - start) and sum of IG of each.

The default dataset is the synthetic stand-in kept as a test fixture (tests/golden/g9_seqcnn.npz, see examples/train_seqcnn.py);
--dataset takes a dataset.jbl written by the sample's 02make_dataset.py.

    python examples/visualize_seqcnn.py [--params FILE] [--epochs 2] [--dataset dataset.jbl] [--out viz_cnn] [--ig-label-target 1]
                                        [--method ig|grad_prod|grad|smooth_grad|smooth_ig] [--divide-number 100] [--noise-scale 0.1]
                                        [--seed 1234] [--proteins positives|all] [--limit N] [--header mol] [--fused | --composed]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kgcn_amd import data_util as D, models, train, visualization as V  # noqa: E402


def short_fit(model, tokens, label, epochs, batch=8, lr=1e-3):
    """A few eager epochs over the whole dataset (batch 8, TF-style Adam): enough for the stand-in's planted motif to show."""
    dev, G = tokens.device, tokens.shape[0]
    opt = train.TFAdam(model.parameters(), lr=lr)
    labels = torch.as_tensor(label, device=dev)
    rng = np.random.default_rng(4321)
    history = []
    for _ in range(epochs):
        order, cost = rng.permutation(G), 0.0
        for it in range(0, G - batch + 1, batch):
            idx = torch.as_tensor(order[it:it + batch], device=dev)
            cs, _ = train.train_step(model, opt, model.loss, None, None, labels[idx], torch.ones(batch, device=dev), sequences=tokens[idx])
            cost += float(cs)
        history.append(cost / (G // batch * batch))
    return history


def main(argv=None):
    import joblib
    ap = argparse.ArgumentParser()
    ap.add_argument("--method", default="ig", choices=V.IG_METHODS + V.SMOOTH_METHODS)
    ap.add_argument("--ig-label-target", default="1", help="max, all, label, correct, uncorrect or a class index (03run.sh: 1)")
    ap.add_argument("--divide-number", type=int, default=100)
    ap.add_argument("--noise-scale", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=1234, help="seed of the device noise of smooth_grad / smooth_ig")
    ap.add_argument("--dataset", default=None, help="dataset.jbl of 02make_dataset.py (default: the committed synthetic fixture)")
    ap.add_argument("--params", default=None, help="a state dict examples/train_seqcnn.py --save wrote")
    ap.add_argument("--epochs", type=int, default=2, help="epochs of the short fit when no --params are given")
    ap.add_argument("--proteins", default="positives", choices=("positives", "all"))
    ap.add_argument("--limit", type=int, default=None, help="visualise the first N of the selected proteins only")
    ap.add_argument("--out", default="viz_cnn")
    ap.add_argument("--header", default="mol")
    route = ap.add_mutually_exclusive_group()
    route.add_argument("--fused", action="store_true", help="force the route fused over the copies (fused=True)")
    route.add_argument("--composed", action="store_true", help="run the scaled rows through the model and autograd (fused=False)")
    a = ap.parse_args(argv)

    dev = torch.device("cuda:0")
    raw = joblib.load(a.dataset) if a.dataset else np.load(os.path.join(ROOT, "tests", "golden", "g9_seqcnn.npz"))
    label = np.asarray(raw["label"], np.float32)
    tokens, S = D.sequence_table({"sequence": raw["sequence"], "sequence_symbol_num": raw["sequence_symbol_num"]}, dev)
    torch.manual_seed(0)
    model = models.SeqCNN(S, embedding_dim=25, label_dim=label.shape[1], class_weight=np.asarray(raw["class_weight"])).to(dev)
    with torch.no_grad():
        model(None, None, sequences=tokens[:1])                      # Keras-style build
    if a.params:
        model.load_state_dict(torch.load(a.params, map_location=dev))
        print("parameters loaded from %s" % a.params)
    else:
        hist = short_fit(model, tokens, label, a.epochs)
        print("short fit: %d epochs, training cost per sequence %s" % (a.epochs, " -> ".join("%.5f" % h for h in hist)))
    keep = np.arange(label.shape[0]) if a.proteins == "all" else np.flatnonzero(label.argmax(1) == 1)      # pos_dataset.jbl
    keep = keep[:a.limit]
    sub = tokens[torch.as_tensor(keep, device=dev)].contiguous()
    lt = a.ig_label_target
    label_target = lt if lt in ("max", "all", "label", "correct", "uncorrect") else int(lt)

    os.makedirs(a.out, exist_ok=True)
    torch.cuda.synchronize()
    t0 = time.time()
    results = V.seqcnn_integrated_gradients(model, sub, labels=label[keep], divide_number=a.divide_number, method=a.method,
                                            label_target=label_target, sequence_symbol=np.asarray(raw["sequence"])[keep],
                                            fused=True if a.fused else False if a.composed else None, noise_scale=a.noise_scale,
                                            seed=a.seed)
    elapsed = time.time() - t0
    files = []
    for r in results:
        path = os.path.join(a.out, V.ig_filename(a.header, r["compound_id"], r["assay"], "embedded_layer"))
        with open(path, "wb") as f:
            joblib.dump(V.dump_record(r), f)
        files.append(path)
        print("[SAVE] %s" % path)
        print("No.%d: prediction score: %.6f  check score: %.6f  sum of IG: %.6f  |difference| %.2e"
              % (r["compound_id"], r["prediction_score"], r["check_score"], r["sum_of_IG"], abs(r["check_score"] - r["sum_of_IG"])))
    print("time: %.3f s for %d dumps" % (elapsed, len(results)))
    return files


if __name__ == "__main__":
    main()
