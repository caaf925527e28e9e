#!/usr/bin/env python3
"""kgcn train_cv --config config_mt.json of sample_chem/compound-protein_interaction/run.sh, on the MI355X path: five folds of
the sample's multitask network (multitask.py: GraphConv(512) sigmoid, GraphGather, Dense(2 T), a two-way softmax per task under
mask_label), batch 50, learning rate 1e-3, patience 3, validation rate 0.2, TF-style Adam.  The dataset lives in HBM; one captured
training step and one captured evaluation step serve all folds; the test fold's predictions stay on the device, where
ops.binary_metrics turns them into the sums behind AUC and AP.  Prints the table of the sample's eval.py: task, mean AUC and
standard deviation over the folds; --out writes cv.json.

The sample's multitask.jbl needs RDKit and a download, so the default dataset is the synthetic stand-in of
tests/golden/g11_cv.npz (60 graphs of 10 nodes, 3 tasks whose labels are planted in the features, about 30 % of mask_label
zero); --dataset takes a real .jbl (joblib) with dense_adj | adj, feature, label and mask_label.

    python examples/train_cv.py [--epochs 20] [--folds 5] [--dataset multitask.jbl] [--out cv.json] [--metrics-mask]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kgcn_amd import cv, data_util as D, models  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--epochs", type=int, default=20)
ap.add_argument("--folds", type=int, default=5)
ap.add_argument("--batch", type=int, default=50)
ap.add_argument("--dataset", default=None)
ap.add_argument("--out", default=None)
ap.add_argument("--metrics-mask", action="store_true", help="score only the rows with mask_label != 0 (the reference scores all)")
a = ap.parse_args()

dev = torch.device("cuda:0")
if a.dataset:
    import joblib
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
          "epoch": a.epochs, "shuffle_data": True, "metrics_mask": a.metrics_mask, "save_result_cv": a.out}
out = cv.train_cv(lambda: models.CPIMultitaskNet(len(channels), T), dataset, label, mask_label, config)
for fold, info in enumerate(out["info_cv"], 1):
    print("fold %d: %2d epochs (best %s), training cost %.4f -> %.4f, test cost %.4f, test accuracy %.4f, fit %.2f s"
          % (fold, len(info["training_cost"]), info["best_epoch"], info["training_cost"][0], info["training_cost"][-1],
             info["test_cost"], info["test_acc"], info["train_time"]))
print("task\tauc(mean)\tauc(std)")
for task, mean, std in cv.auc_table(out["result_cv"]):
    print("%d\t%.4f\t%.4f" % (task, mean, std))
