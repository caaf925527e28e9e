#!/usr/bin/env python3
"""graph_kernel/gk.py --kernel wl|sp on the MI355X path: the Weisfeiler-Lehman subtree (3 iterations) or shortest-path Gram matrix
of a data set on the device (kgcn_amd.graph_kernel), normalised, then the nested k-fold SVM of gk.py: --svm host (the default;
scikit-learn, one fit after another) or --svm device (all fits as one batch of the HIP solver; the Gram never leaves the device
before the SVM; the two agree to the solver's tolerance --svm-tol, not bit for bit).
--kernel hgk-wl|hgk-sp: the hash graph kernel over the data set's continuous node attributes ("feature" [T, M, F]) with the WL or
SP base kernel (graphkernel/hash_graph_kernel.py): --hash-iterations draws seeded by --seed, buckets --bin-width wide, --use-labels
none (the hashes alone) | node | degree (joint (label, hash) classes).
Saves gram_wl.npy / gram_sp.npy / gram_hgk_wl.npy / gram_hgk_sp.npy and label.npy into --output and prints the accuracy table.
Without --input_dataset the two-class stand-in set of tests/golden/g13_graph_kernel.npz (120 graphs, ring-rich against tree-like)
is used, for hgk-* with the attributes of tests/golden/g14_hash_kernel.npz.  The data set is shuffled with --seed; --limit cuts it
after the shuffle (default: no cut; the reference cuts at 3,000).

    python examples/graph_kernel.py --kernel wl|sp|hgk-wl|hgk-sp [--input_dataset X.jbl] [--limit N] [--output DIR]
        [--test_splits 5] [--seed 0] [--hash-iterations 20] [--bin-width 1.0] [--sigma 1.0] [--use-labels none|node|degree]
        [--svm host|device] [--svm-tol 1e-3]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kgcn_amd import graph_kernel as gk  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--kernel", choices=("wl", "sp", "hgk-wl", "hgk-sp"), default="wl")
ap.add_argument("--input_dataset", default=None, help="joblib file of a kGCN data set (adj or dense_adj, node, feature, label)")
ap.add_argument("--limit", type=int, default=0, help="use the first N graphs after the shuffle (0: all)")
ap.add_argument("--output", default=".")
ap.add_argument("--test_splits", type=int, default=5)
ap.add_argument("--seed", type=int, default=0, help="of the shuffle and of the hash kernels' projections")
ap.add_argument("--hash-iterations", type=int, default=20, help="hgk-*: random projections R")
ap.add_argument("--bin-width", type=float, default=1.0, help="hgk-*: bucket width w")
ap.add_argument("--sigma", type=float, default=1.0, help="hgk-*: scale of the projections")
ap.add_argument("--use-labels", choices=("none", "node", "degree"), default="none", help="hgk-*: discrete labels beside the hashes")
ap.add_argument("--svm", choices=("host", "device"), default="host", help="where the nested-CV SVMs are fitted")
ap.add_argument("--svm-tol", type=float, default=1e-3, help="stopping tolerance of the SVM solver (SVC's tol)")
a = ap.parse_args()
hashed = a.kernel.startswith("hgk-")

attrs = None
if a.input_dataset is None:
    z = np.load(os.path.join(ROOT, "tests", "golden", "g13_graph_kernel.npz"), allow_pickle=False)
    nn, eo, edges = z["two_num_nodes"], z["two_edge_offsets"], z["two_edges"]
    lo = np.concatenate([[0], np.cumsum(nn)])
    M = int(nn.max())
    adjs = [[(edges[eo[g]:eo[g + 1]].astype(np.int64), np.ones(eo[g + 1] - eo[g], np.float32), (M, M))] for g in range(len(nn))]
    labels = [z["two_labels"][lo[g]:lo[g + 1]] for g in range(len(nn))]
    y = z["two_y"]
    if hashed:
        rows = np.load(os.path.join(ROOT, "tests", "golden", "g14_hash_kernel.npz"), allow_pickle=False)["two_attr"]
        attrs = np.zeros((len(nn), M, rows.shape[1]))
        for g in range(len(nn)):
            attrs[g, :nn[g]] = rows[lo[g]:lo[g + 1]]
else:
    import joblib
    obj = joblib.load(a.input_dataset)
    adjs, nn, labels, y = gk.dataset_graphs(obj)
    if hashed:
        attrs = gk.dataset_attributes(obj)
        if attrs is None:
            sys.exit('%s has no "feature" tensor for --kernel %s' % (a.input_dataset, a.kernel))
        if labels is None and a.use_labels == "node":
            sys.exit('%s has no "node" labels for --use-labels node' % a.input_dataset)
    elif labels is None:
        sys.exit('%s has no "node" labels: use --kernel hgk-wl | hgk-sp on its "feature" tensor' % a.input_dataset)
    y = np.asarray(y)
    y = y[:, 0] if y.ndim > 1 else y                                    # gk.py:171
order = np.random.default_rng(a.seed).permutation(len(nn))
if a.limit and len(order) > a.limit:
    print("[WARN] too much data: limited-%d" % a.limit)
    order = order[:a.limit]
adjs, nn, y = [adjs[i] for i in order], np.asarray(nn)[order], y[order]
labels = None if labels is None else [labels[i] for i in order]

if hashed:
    K = gk.hash_graph_kernel(adjs, nn, np.asarray(attrs)[order], base=a.kernel[4:], node_labels=labels,
                             labels=None if a.use_labels == "none" else a.use_labels, hash_iterations=a.hash_iterations,
                             wl_iterations=3, bin_width=a.bin_width, sigma=a.sigma, seed=a.seed)
else:
    kernel = gk.wl_subtree_kernel if a.kernel == "wl" else gk.shortest_path_kernel
    K = kernel(adjs, nn, labels, iterations=3)
if a.svm == "device":                                                   # the SVM reads the Gram where it was built
    res = gk.svm_cv(K, y, test_splits=a.test_splits, device=True, tol=a.svm_tol)
K = K.cpu().numpy()
os.makedirs(a.output, exist_ok=True)
for name, arr in (("gram_%s.npy" % a.kernel.replace("-", "_"), K), ("label.npy", y)):
    print("[SAVE] " + os.path.join(a.output, name))
    np.save(os.path.join(a.output, name), arr)

if a.svm == "host":
    res = gk.svm_cv(K, y, test_splits=a.test_splits, device=False, tol=a.svm_tol)
print("%d graphs, %s kernel, SVM on the %s" % (len(y), a.kernel, a.svm))
print("split  best C     acc. (validation)  acc. (test)")
for k, (c, v, t) in enumerate(zip(res["best_C"], res["val_acc"], res["test_acc"])):
    print("%5d  %-9.4f %-18.6f %.6f" % (k, c, v, t))
print("=======================")
print("Accuracy (test) mean: %3f" % res["mean"])
print("Accuracy (test) std.: %3f" % res["std"])
