#!/usr/bin/env python3
"""active_learning/README.md's usage on this path (kgcn_amd/active_learning.py): simulate --n queries of an ActiveLearner over a pool
whose labels are known, and print, per query, the ORIGINAL pool index that was picked and the accuracy of the label propagation
on the rows still in the pool (mean over tasks).  Default data: the 257-point, three-task set of
tests/golden/g16_active_learning.npz (its first 40 rows are the training set).

    python examples/active_learning.py [--algorithm LP|LS] [--strategy E|LC|MS|RS|all] [--gamma G] [--n 10] [--seed 0]
                                        [--matrix-free off|on|auto]

--matrix-free on never stores the affinity matrix (its tiles are rebuilt where they are used; the same picks and accuracies, bit
for bit), auto stores it when it fits the estimator's max_bytes.  --gamma defaults to 1 / d on the standardised points (the reference's own default, 20, leaves these points unconnected)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kgcn_amd import active_learning as al, ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--algorithm", choices=("LP", "LS"), default="LS")
ap.add_argument("--strategy", choices=("E", "LC", "MS", "RS", "all"), default="all")
ap.add_argument("--gamma", type=float, default=None)
ap.add_argument("--n", type=int, default=10)
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--matrix-free", choices=("off", "on", "auto"), default="off")
a = ap.parse_args()

z = np.load(os.path.join(ROOT, "tests", "golden", "g16_active_learning.npz"))
X, truth, m = z["n257_X"], z["n257_truth"], int(z["loop_train"])
gamma = 1.0 / X.shape[1] if a.gamma is None else a.gamma


def estimator():
    est = al.LabelSpreading(gamma=gamma) if a.algorithm == "LS" else al.LabelPropagation(gamma=gamma)
    est.matrix_free = {"off": False, "on": True, "auto": "auto"}[a.matrix_free]
    return est


def pool_accuracy(learner, X_pool, Y_pool):
    """Fit all tasks over [training; pool] (standardised as ActiveLearner.query standardises) and compare the pool's transduction."""
    import torch
    Xs = ops.attr_scale(torch.from_numpy(np.vstack([learner.X_training_vectors, X_pool])).cuda())[0]
    Y = np.vstack([learner.Y_training, np.full_like(Y_pool, -1)])
    model = estimator().fit_tasks(Xs, Y)
    n_train = len(learner.Y_training)
    return float(np.mean([np.mean(t[n_train:] == Y_pool[:, k]) for k, t in enumerate(model.transduction_)]))


for strategy in (("E", "LC", "MS", "RS") if a.strategy == "all" else (a.strategy,)):
    learner = al.ActiveLearner(estimator(), X[:m], truth[:m], query_strategy=strategy, seed=a.seed)
    X_pool, Y_pool, left = X[m:], truth[m:], list(range(len(X) - m))
    print("%s, strategy %s, gamma %.4g: %d training rows, %d in the pool, accuracy %.4f"
          % (a.algorithm, strategy, gamma, m, len(left), pool_accuracy(learner, X_pool, Y_pool)))
    for q in range(a.n):
        p = learner.query_and_teach_n_times(1, X_pool, Y_pool)[0]
        X_pool, Y_pool = np.delete(X_pool, p, axis=0), np.delete(Y_pool, p, axis=0)
        print("  query %2d: pool row %3d taught, accuracy on the %d left %.4f" % (q + 1, left.pop(p), len(left), pool_accuracy(learner, X_pool, Y_pool)))
