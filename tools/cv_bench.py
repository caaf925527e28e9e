#!/usr/bin/env python3
"""The cross-validation workflow (examples/train_cv.py) in numbers, one JSON line:
  step      the captured training step and the captured evaluation step of models.CPIMultitaskNet at batch 50 on the stand-in
            dataset (tests/golden/g11_cv.npz: 10 nodes, 8 features, 3 tasks): median wall time of 200 replays between device
            synchronisations, staging of the batch indices included
  fold      one fold of cv.CrossValidator (hold-out split, fit with early stopping, test fold scored, metrics) on the stand-in
            dataset tiled to --graphs graphs, --epochs epochs: wall time, and the part of it spent in ops.binary_metrics
  metrics   ops.binary_metrics at n in {1e3, 1e5, 1e6} x T = 4 (scores quantised to 1000 levels: ties in every task): wall
            time of the call, read-back included, beside the same sums by numpy on the host (stable argsort + cumsum per task,
            from host arrays: the copy of the predictions off the device is not charged to it); the integers must agree
usage: python tools/cv_bench.py [--steps K] [--graphs G] [--epochs E] [--out profiles/cv_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kgcn_amd import cv, data_util as D, models, ops  # noqa: E402

dev = torch.device("cuda:0")


def wall(fn, steps, warmup=3):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def host_sums(score, label, threshold=0.5):
    """n_used, P, TP, FP, auc_num2, n_groups and ap of every task with numpy (vectorised)."""
    rows = []
    for t in range(score.shape[1]):
        s, l = score[:, t], label[:, t] != 0
        order = np.argsort(-s, kind="stable")
        s, l = s[order], l[order]
        ends = np.r_[np.nonzero(s[1:] != s[:-1])[0], len(s) - 1]
        tp = np.cumsum(l)[ends].astype(np.int64)
        fp = ends + 1 - tp
        tp0, fp0 = np.r_[0, tp[:-1]], np.r_[0, fp[:-1]]
        P = int(l.sum())
        above = score[:, t] > np.float32(threshold)
        ap = float((((tp - tp0) / P) * (tp / (tp + fp))).sum()) if P else 0.0
        rows.append(([len(s), P, int((above & (label[:, t] != 0)).sum()), int((above & (label[:, t] == 0)).sum()), 0,
                      int(((fp - fp0) * (tp + tp0)).sum()), len(ends), 0], ap))
    return np.array([r[0] for r in rows], np.int64), np.array([r[1] for r in rows])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--graphs", type=int, default=6000)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    z = np.load(os.path.join(ROOT, "tests", "golden", "g11_cv.npz"))
    reps = max(1, a.graphs // z["ds_label"].shape[0])
    tile = lambda v: np.concatenate([v] * reps)
    channels, _ = D.build_adjs({"dense_adj": tile(z["ds_dense_adj"]), "max_node_num": int(z["ds_max_node_num"])})
    ds = D.DeviceGraphDataset(channels, tile(z["ds_feature"]), device=dev)
    label, mask = tile(z["ds_label"]), tile(z["ds_mask_label"])
    G, T = label.shape
    v = cv.CrossValidator(lambda: models.CPIMultitaskNet(len(channels), T), ds, label, mask, {"epoch": a.epochs, "patience": 0})
    rng = np.random.default_rng(0)
    idx = rng.permutation(G)[:50]

    def train_step():
        v.batch.stage(idx)
        v.step.replay()

    def eval_step():
        v.batch.stage(idx)
        v.eval_graph.replay()

    step = dict(batch=50, train_ms=wall(train_step, a.steps), eval_ms=wall(eval_step, a.steps))
    folds = cv.kfold_indices(G, 5)
    spent = [0.0]
    inner = ops.binary_metrics

    def timed(*args, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = inner(*args, **kw)
        spent[0] += time.perf_counter() - t0
        return out

    ops.binary_metrics = timed
    try:
        v.run_fold(1, *folds[0])                                    # warm
        spent[0] = 0.0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, info, _ = v.run_fold(1, *folds[0])
        torch.cuda.synchronize()
        fold_s = time.perf_counter() - t0
    finally:
        ops.binary_metrics = inner
    fold = dict(graphs=G, epochs=len(info["training_cost"]), train_graphs=len(folds[0][0]), test_graphs=len(folds[0][1]),
                fold_s=fold_s, fit_s=info["train_time"], binary_metrics_ms=spent[0] * 1e3)

    metrics = []
    for n in (1000, 100000, 1000000):
        score = (np.round(rng.random((n, 4)) * 999) / 999).astype(np.float32)
        lab = (rng.random((n, 4)) < 0.3).astype(np.float32)
        ts, tl = torch.as_tensor(score, device=dev), torch.as_tensor(lab, device=dev)
        dev_ms = wall(lambda: ops.binary_metrics(ts, tl), 10 if n < 1000000 else 5)
        counts, apv = ops.binary_metrics(ts, tl)
        t0 = time.perf_counter()
        want, want_ap = host_sums(score, lab)
        host_ms = (time.perf_counter() - t0) * 1e3
        metrics.append(dict(n=n, tasks=4, device_ms=dev_ms, host_numpy_ms=host_ms, integers_equal=bool((counts == want).all()),
                            max_ap_diff=float(np.abs(apv - want_ap).max())))
    res = dict(step=step, fold=fold, metrics=metrics, device=torch.cuda.get_device_name(0))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
