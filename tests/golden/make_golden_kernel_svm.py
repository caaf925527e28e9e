#!/usr/bin/env python
"""Generate tests/golden/g15_kernel_svm.npz by RUNNING scikit-learn's SVC(kernel="precomputed") -- the solver graph_kernel/gk.py:243-292
of the reference calls -- over the two normalised Gram matrices of g13_graph_kernel.npz (two_wl_node_norm; two_sp_node_norm, which
has a zero eigenvalue and duplicate graphs) on the 5 x 5 nested folds and the five C of gk.py.  Arrays and recorded results only.

  sklearn_version, tol (1e-10), C_grid [5]
  train_ptr / train_idx, val_ptr / val_idx, test_ptr / test_idx     the 25 fits' index sets (outer split major), KFold unshuffled
  y2 [120] the two classes of g13 (two_y); y3 [120] three classes: y2 == 0 | y2 == 1 with fewer than 14 nodes | the rest
  for gram in (wl, sp) and lab in (y2, y3), rows ordered fit, C, (validation, test), row:
    <gram>_<lab>_dec     decision_function at tol: y2 [rows] scikit-learn's sign; y3 [rows, 3] one-vs-one (decision_function_shape="ovo")
    <gram>_<lab>_pred    predict
    <gram>_<lab>_acc     [25, 5, 2] accuracy_score on the validation and the test rows
    <gram>_<lab>_cv_*    kgcn_amd.graph_kernel.svm_cv(device=False, tol=tol): best_C, val_acc, test_acc [5], mean, std
The generator asserts that on y3 the nested-CV mean beats the majority class.

    python tests/golden/make_golden_kernel_svm.py
"""
import os
import sys

import numpy as np
import sklearn
from sklearn.metrics import accuracy_score
from sklearn.model_selection import KFold
from sklearn.svm import SVC

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
TOL = 1e-10


def nested_folds(n):
    out = []
    for tv, te in KFold(n_splits=5).split(np.arange(n)):
        for a, b in KFold(n_splits=5).split(tv):
            out.append((tv[a], tv[b], te))
    return out


def packed(sets):
    return np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64), np.concatenate(sets).astype(np.int64)


def main():
    from kgcn_amd import graph_kernel as gk
    g13 = np.load(os.path.join(HERE, "g13_graph_kernel.npz"))
    y2 = g13["two_y"].astype(np.int64)
    y3 = np.where(y2 == 0, 0, np.where(g13["two_num_nodes"] < 14, 1, 2)).astype(np.int64)
    folds = nested_folds(120)
    C_grid = np.linspace(1e-4, 10, 5)
    z = {"sklearn_version": np.array(sklearn.__version__), "tol": np.float64(TOL), "C_grid": C_grid, "y2": y2, "y3": y3}
    for name, which in (("train", 0), ("val", 1), ("test", 2)):
        z[name + "_ptr"], z[name + "_idx"] = packed([f[which] for f in folds])
    for gram, key in (("wl", "two_wl_node_norm"), ("sp", "two_sp_node_norm")):
        K = g13[key]
        for lab, y in (("y2", y2), ("y3", y3)):
            decs, preds, acc = [], [], np.zeros((len(folds), len(C_grid), 2))
            for f, (tr, va, te) in enumerate(folds):
                for c, C in enumerate(C_grid):
                    clf = SVC(kernel="precomputed", C=float(C), tol=TOL, decision_function_shape="ovo").fit(K[np.ix_(tr, tr)], y[tr])
                    assert clf.fit_status_ == 0
                    for e, rows in enumerate((va, te)):
                        block = K[np.ix_(rows, tr)]
                        decs.append(clf.decision_function(block))
                        preds.append(clf.predict(block))
                        acc[f, c, e] = accuracy_score(y[rows], preds[-1])
            z["%s_%s_dec" % (gram, lab)] = np.concatenate(decs).astype(np.float64)
            z["%s_%s_pred" % (gram, lab)] = np.concatenate(preds).astype(np.int64)
            z["%s_%s_acc" % (gram, lab)] = acc
            cv = gk.svm_cv(K, y, device=False, tol=TOL)
            for k in ("best_C", "val_acc", "test_acc", "mean", "std"):
                z["%s_%s_cv_%s" % (gram, lab, k)] = np.asarray(cv[k], np.float64)
            majority = np.bincount(y).max() / len(y)
            print("%s %s: nested-CV mean %.4f (majority class %.4f), best C %s" % (gram, lab, cv["mean"], majority, cv["best_C"]))
            if lab == "y3":
                assert cv["mean"] > majority, (cv["mean"], majority)
    out = os.path.join(HERE, "g15_kernel_svm.npz")
    np.savez_compressed(out, **z)
    print("wrote", out, os.path.getsize(out), "bytes")
    write_bounds()


def write_bounds():
    """g15_kernel_svm_bounds.json: the measured distance of the fp64 restatement (tests/kernel_svm_oracle.py) from the recorded
    decisions, per Gram and per C, over every row of every fit of both labellings; how many reference rows a bound of ten times
    that distance leaves undecided; per_C: whether that is past 2 % of the rows, so that the tests apply the bound C by C."""
    import json
    sys.path.insert(0, os.path.dirname(HERE))
    import kernel_svm_cases as cases
    doc = {"sklearn_version": sklearn.__version__, "tol": TOL, "bound_factor": cases.BOUND_FACTOR}
    for gram in ("wl", "sp"):
        overall, per_c = cases.distances(gram)
        one = [cases.left_out(gram, lab, [cases.BOUND_FACTOR * overall] * len(per_c)) for lab in ("y2", "y3")]
        by_c = [cases.left_out(gram, lab, cases.BOUND_FACTOR * per_c) for lab in ("y2", "y3")]
        per = any(n > cases.LEFT_OUT_CAP * total for n, total in one)
        doc[gram] = {"distance": overall, "distance_per_C": [float(v) for v in per_c], "per_C": bool(per),
                     "left_out_one_bound": {"y2": one[0], "y3": one[1]}, "left_out_per_C": {"y2": by_c[0], "y3": by_c[1]}}
        print(gram, doc[gram])
    with open(cases.BOUNDS, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
