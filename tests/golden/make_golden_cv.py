#!/usr/bin/env python3
"""Writes tests/golden/g11_cv.npz: what scikit-learn answers where `kgcn train_cv` calls it, and the stand-in dataset of
examples/train_cv.py.  Needs scikit-learn (1.7.2 when the committed file was made); the tests read the file, never scikit-learn.

  kf{i}_*      KFold(n_splits=k, shuffle=s, random_state=123).split (gcn.py:364, 382) for (n, k, s) of KFOLD_CASES
  ho_*         split_data's shuffle-and-cut (kgcn/data_util.py:612-618) under RandomState(5), n = 48, rate 0.2
  m{j}_*       label / score cases with every metric of compute_metrics, the calls of gcn.py:210-227 in that order; the
               scores are float32, as a prediction comes off the network
  ds_*         60 graphs of 10 nodes, 8 features, 3 tasks: label[g, t] is planted in the mean of feature column t, about 30 % of
               mask_label is 0 and graph 0 has every task masked

    python tests/golden/make_golden_cv.py
"""
import os
import warnings

import numpy as np
from sklearn.metrics import (accuracy_score, auc, average_precision_score, balanced_accuracy_score, jaccard_score, matthews_corrcoef,
                             precision_recall_fscore_support, roc_curve)
from sklearn.model_selection import KFold

HERE = os.path.dirname(os.path.abspath(__file__))
KFOLD_CASES = ((23, 5, True), (10, 5, True), (7, 3, True), (12, 4, False))
METRIC_KEYS = ("auc", "acc", "ap", "pre", "rec", "f", "balanced_acc", "mcc", "jaccard")


def compute_metrics(true_label, pred_score):
    """gcn.py:210-227 for one task."""
    pred = np.zeros(pred_score.shape)
    pred[pred_score > 0.5] = 1
    fpr, tpr, _ = roc_curve(true_label, pred_score, pos_label=1)
    el = {"auc": auc(fpr, tpr)}
    el["ap"] = average_precision_score(true_label, pred_score, pos_label=1)
    el["acc"] = accuracy_score(true_label, pred)
    scores = precision_recall_fscore_support(true_label, pred, average="binary")
    el["pre"], el["rec"], el["f"] = scores[0], scores[1], scores[2]
    assert scores[3] is None                                    # `sup` of average='binary'
    el["balanced_acc"] = balanced_accuracy_score(true_label, pred)
    el["mcc"] = matthews_corrcoef(true_label, pred)
    el["jaccard"] = jaccard_score(true_label, pred)
    return np.array([el[k] for k in METRIC_KEYS], np.float64)


def metric_cases(rng):
    def lab(n, p=0.4):
        v = (rng.random(n) < p).astype(np.int64)
        v[0], v[1] = 0, 1
        return v

    cases = []
    n = 50
    cases.append(("continuous", lab(n), rng.random(n)))
    y = lab(200)
    cases.append(("heavy_ties", y, np.round((rng.random(200) * 0.6 + 0.25 * y) * 4) / 4))
    cases.append(("all_equal", lab(40), np.full(40, 0.625)))
    s = rng.random(30) - 0.5
    s[:6] = [0.0, -0.0, 0.0, -0.0, -0.0, 0.0]
    y = lab(30)
    y[:6] = [1, 0, 0, 1, 1, 0]
    cases.append(("signed_zero", y, s))
    cases.append(("no_positives", np.zeros(25, np.int64), rng.random(25)))
    cases.append(("no_negatives", np.ones(25, np.int64), rng.random(25)))
    cases.append(("no_predicted_positives", lab(35), rng.random(35) * 0.5))
    cases.append(("all_predicted_positive", lab(35), 0.5 + rng.random(35) * 0.49 + 0.005))
    y = lab(64)
    cases.append(("separated", y, np.where(y == 1, 0.9, 0.1) + rng.random(64) * 0.05))
    cases.append(("inverted", y, np.where(y == 1, 0.1, 0.9) + rng.random(64) * 0.05))
    y = lab(1000, 0.1)
    cases.append(("quantised_1000", y, np.round((rng.random(1000) * 0.8 + 0.2 * y) * 1000) / 1000))
    cases.append(("two_rows", np.array([0, 1]), np.array([0.7, 0.7])))
    cases.append(("denormal", lab(20), rng.integers(1, 1 << 20, 20).astype(np.uint32).view(np.float32)))
    cases.append(("at_threshold", lab(40), np.where(rng.random(40) < 0.5, 0.5, rng.random(40))))
    return [(name, y.astype(np.int64), np.asarray(s, np.float32)) for name, y, s in cases]


def dataset(rng):
    G, N, F, T = 60, 10, 8, 3
    sizes = rng.integers(5, N + 1, G)
    adj = np.zeros((G, N, N), np.float32)
    feat = np.zeros((G, N, F), np.float32)
    for g, m in enumerate(sizes):
        for i in range(m):                                       # a ring with self loops and two chords
            adj[g, i, i] = adj[g, i, (i + 1) % m] = adj[g, (i + 1) % m, i] = 1.0
        for _ in range(2):
            i, j = rng.integers(0, m, 2)
            adj[g, i, j] = adj[g, j, i] = 1.0
        feat[g, :m] = rng.standard_normal((m, F))
    label = np.zeros((G, T), np.float32)
    for t in range(T):
        want = rng.random(G) < 0.5
        label[:, t] = want
        for g, m in enumerate(sizes):                            # the pattern: the mean of column t says the label
            feat[g, :m, t] += 1.5 if want[g] else -1.5
    mask = (rng.random((G, T)) >= 0.3).astype(np.float32)
    mask[0] = 0.0
    mask[1] = 1.0
    return {"ds_dense_adj": adj, "ds_feature": feat, "ds_label": label, "ds_mask_label": mask, "ds_sizes": sizes.astype(np.int64),
            "ds_max_node_num": np.int64(N)}


def main():
    out = {}
    for i, (n, k, s) in enumerate(KFOLD_CASES):
        kf = KFold(n_splits=k, shuffle=s, random_state=123 if s else None)
        base = np.zeros((n, 2))
        out["kf%d_nks" % i] = np.array([n, k, int(s)], np.int64)
        for f, (tr, te) in enumerate(kf.split(base)):
            out["kf%d_train%d" % (i, f)] = np.asarray(tr, np.int64)
            out["kf%d_test%d" % (i, f)] = np.asarray(te, np.int64)
    out["kf_cases"] = np.int64(len(KFOLD_CASES))
    # split_data (kgcn/data_util.py:612-618) with the process-wide numpy state seeded
    num, rate = 48, 0.2
    np.random.seed(5)
    valid_num = int(num * rate)
    train_num = num - valid_num
    indices = np.arange(num)
    np.random.shuffle(indices)
    out["ho_args"] = np.array([num, 5], np.int64)
    out["ho_rate"] = np.float64(rate)
    out["ho_train"], out["ho_valid"] = indices[:train_num], indices[train_num:num]
    rng = np.random.default_rng(11)
    cases = metric_cases(rng)
    names = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for j, (name, y, s) in enumerate(cases):
            names.append(name)
            out["m%d_label" % j], out["m%d_score" % j] = y, s
            out["m%d_metrics" % j] = compute_metrics(y, s)
    out["m_names"] = np.array(names)
    out["m_keys"] = np.array(METRIC_KEYS)
    out.update(dataset(np.random.default_rng(12)))
    import sklearn
    out["sklearn_version"] = np.array(sklearn.__version__)
    np.savez_compressed(os.path.join(HERE, "g11_cv.npz"), **out)
    print("wrote g11_cv.npz: %d KFold cases, %d metric cases, %d graphs" % (len(KFOLD_CASES), len(cases), out["ds_label"].shape[0]))


if __name__ == "__main__":
    main()
