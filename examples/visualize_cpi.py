#!/usr/bin/env python3
"""kgcn visualize of sample_chem/compound-protein_interaction/run_viz.sh (block name=mt), on the MI355X path: integrated gradients
of the multitask network (multitask.py, models.CPIMultitaskNet) over the node features and the channel-0 adjacency values, for
the test compounds of one cross-validation fold and every task.  Trains that fold with the setup of examples/train_cv.py (batch
50, learning rate 1e-3, patience 3, validation rate 0.2; --epochs), or loads the fold's saved best parameters (--params
model.<fold>.best.pt, the flat vector cv.CrossValidator.fit writes under save_model_path).  Writes one
{header}_{id:04d}_task_{t}_{assay}_{modal}_scaling.jbl per (compound, task) (joblib, the keys kgcn/visualization.py dumps) and
logs the prediction score, check score (end - start) and sum of IG of each.

The default dataset is the synthetic stand-in of tests/golden/g11_cv.npz (60 graphs of 10 nodes, 3 tasks); --dataset takes a
real .jbl (joblib) with dense_adj | adj, feature, label and mask_label.

    python examples/visualize_cpi.py [--fold 1] [--folds 5] [--epochs 20] [--params FILE] [--save-model DIR] [--outdir viz_cpi]
                                     [--modal all|features|adjs] [--method ig|grad_prod|grad] [--label-target max]
                                     [--divide-number 100] [--header mol] [--composed]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kgcn_amd import cv, data_util as D, models, visualization as V  # noqa: E402


def main(argv=None):
    import joblib
    ap = argparse.ArgumentParser()
    ap.add_argument("--fold", type=int, default=1, help="the fold whose test compounds are visualised (1-based)")
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=20, help="training epochs when no --params are given")
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--dataset", default=None)
    ap.add_argument("--params", default=None, help="model.<fold>.best.pt of a cross-validation run")
    ap.add_argument("--save-model", default=None, help="directory for the trained fold's model.<fold>.best.pt / .last.pt")
    ap.add_argument("--outdir", default="viz_cpi")
    ap.add_argument("--modal", default="all", choices=("all",) + V.CPI_IG_MODALS)
    ap.add_argument("--method", default="ig", choices=V.IG_METHODS)
    ap.add_argument("--label-target", default="max")
    ap.add_argument("--divide-number", type=int, default=100)
    ap.add_argument("--header", default="mol")
    ap.add_argument("--composed", action="store_true", help="run the copies through the model and autograd (fused=False)")
    a = ap.parse_args(argv)

    dev = torch.device("cuda:0")
    if a.dataset:
        raw = joblib.load(a.dataset)
        channels, _ = D.build_adjs(raw)
        feature, label = np.asarray(raw["feature"], np.float32), np.asarray(raw["label"], np.float32)
        mask_label = np.asarray(raw["mask_label"], np.float32) if raw.get("mask_label") is not None else np.ones_like(label)
    else:
        raw = np.load(os.path.join(ROOT, "tests", "golden", "g11_cv.npz"))
        channels, _ = D.build_adjs({"dense_adj": raw["ds_dense_adj"], "max_node_num": int(raw["ds_max_node_num"])})
        feature, label, mask_label = raw["ds_feature"], raw["ds_label"], raw["ds_mask_label"]
    dataset = D.DeviceGraphDataset(channels, feature, device=dev)
    T = label.shape[1]
    config = {"batch_size": a.batch, "learning_rate": 1e-3, "patience": 3, "k-fold_num": a.folds, "validation_data_rate": 0.2,
              "epoch": a.epochs, "shuffle_data": True, "save_model_path": a.save_model}
    validator = cv.CrossValidator(lambda: models.CPIMultitaskNet(len(channels), T), dataset, label, mask_label, config)
    cfg = validator.config
    folds = cv.kfold_indices(dataset.num_graphs, cfg["k-fold_num"], cfg["shuffle_data"], stratified=cfg["stratified_kfold"])
    if not 1 <= a.fold <= len(folds):
        raise SystemExit("--fold must lie in 1..%d" % len(folds))
    train_valid_idx, test_idx = folds[a.fold - 1]
    if a.params:
        validator.restore(torch.load(a.params, map_location=dev))
        print("parameters loaded from %s" % a.params)
    else:
        _, info, _ = validator.run_fold(a.fold, train_valid_idx, test_idx)
        print("fold %d: %d epochs (best %s), test cost %.4f, test accuracy %.4f"
              % (a.fold, len(info["training_cost"]), info["best_epoch"], info["test_cost"], info["test_acc"]))
    model = validator.model

    os.makedirs(a.outdir, exist_ok=True)
    torch.cuda.synchronize()
    t0 = time.time()
    results = V.cpi_integrated_gradients(model, None, dataset, labels=label, divide_number=a.divide_number, modal=a.modal,
                                         method=a.method, label_target=a.label_target, compounds=[int(i) for i in test_idx],
                                         fused=not a.composed)
    elapsed = time.time() - t0
    files = []
    for r in results:
        name = os.path.join(a.outdir, V.ig_filename(a.header, r["compound_id"], r["assay"], a.modal, task=r["task"]))
        with open(name, "wb") as f:
            joblib.dump(V.cpi_dump_record(r), f)
        files.append(name)
        print("[SAVE] %s" % name)
        print("No.%d task %d: prediction score: %.6f  check score: %.6f  sum of IG: %.6f  |difference| %.2e"
              % (r["compound_id"], r["task"], r["prediction_score"], r["check_score"], r["sum_of_IG"],
                 abs(r["check_score"] - r["sum_of_IG"])))
    print("time: %.3f s for %d dumps of %d compounds (%s route)" % (elapsed, len(results), len(test_idx),
                                                                    "composed" if a.composed else "fused"))
    return files


if __name__ == "__main__":
    main()
