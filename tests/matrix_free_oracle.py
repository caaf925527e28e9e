"""numpy restatements for the matrix-free label-propagation tests, beside tests/active_learning_oracle.py (which stays as it is):
the rectangular product in the device's order, scikit-learn's predict_proba, and the cases of tests/golden/g17_lp_predict.npz
(written by tools/gen_lp_predict_golden.py with scikit-learn 1.7.2)."""
import functools
import os

import numpy as np

import active_learning_cases as cases
import active_learning_oracle as O

PREDICT_SETS = ((65, 3), (257, 8))
PREDICT_CASES = ["n%d_%s_%s_c%d" % (n, g, a, c) for n, _ in PREDICT_SETS for g in cases.GAMMAS for a in cases.ALGS for c in range(3)]


@functools.lru_cache(None)
def predict_fixture():
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g17_lp_predict.npz")) as z:
        return {k: z[k] for k in z.files}


def case_parts(case):
    """-> (the g16 tag, the set's key, gamma, the algorithm, the label column)."""
    tag, col = case.rsplit("_c", 1)
    key, n, d, gamma, alg, variant = cases.parts(tag)
    return tag, key, gamma, alg, int(col)


def product_rect(W, G):
    """raw [m, K] = sum_j W_ij G_jc for W [m, n]: lane l adds the rounded products of j = l, l + 64, ... ascending from +0.0, then
    the lane tree (O.product, which takes a square W only)."""
    m, n = W.shape
    K = G.shape[1]
    chunks = -(-n // 64)
    Wp = np.zeros((m, chunks * 64))
    Wp[:, :n] = W
    Gp = np.zeros((chunks * 64, K))
    Gp[:n] = G
    acc = np.zeros((m, 64, K))
    for c in range(chunks):
        acc = acc + Wp[:, c * 64:(c + 1) * 64, None] * Gp[None, c * 64:(c + 1) * 64, :]
    return O._lane_tree(acc)


def rbf_kernel(Xq, Xr, gamma):
    """sklearn.metrics.pairwise.rbf_kernel(Xq, Xr, gamma) for two different sets: no diagonal rule."""
    Xq, Xr = np.asarray(Xq, np.float64), np.asarray(Xr, np.float64)
    dist = ((Xq * Xq).sum(axis=1)[:, None] + (Xr * Xr).sum(axis=1)[None, :]) - 2.0 * (Xq @ Xr.T)
    return np.exp(-gamma * np.maximum(dist, 0.0))


def predict_proba(X_fit, dist, Xq, gamma):
    """BaseLabelPropagation.predict_proba: rbf_kernel(Xq, X_) . label_distributions_, each row divided by its sum; no zero guard."""
    raw = rbf_kernel(Xq, X_fit, gamma) @ dist
    with np.errstate(divide="ignore", invalid="ignore"):
        return raw / raw.sum(axis=1)[:, None]
