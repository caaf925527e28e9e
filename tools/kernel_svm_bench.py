#!/usr/bin/env python3
"""The nested-CV SVMs of graph_kernel/gk.py:243-292 on the device (kgcn_amd.graph_kernel.svm_cv(device=True): csrc/svm.hip) against
the host route (scikit-learn), one JSON record per data set: the normalised WL Gram (3 iterations) of the two-class fixture of
tests/golden/g13_graph_kernel.npz (120 graphs) and of synthetic 50-node graphs (the generator of tools/graph_kernel_bench.py; the
class is whether a graph holds more than the median number of nodes of the three rare labels) at 1,000 and 3,000 graphs, with gk.py's
defaults: 5 x 5 folds, C in linspace(1e-4, 10, 5), tol 1e-3 -- 125 fits.

Device route: the wall time of the whole svm_cv call (median, minimum, maximum over --steps repeats after --warmup) and of its
stages between device synchronisations -- the SMO launches (with the number of launches, the iterations of the longest problem and of
all problems, and the microseconds an iteration of the longest problem took: the launches last as long as their slowest workgroup),
the decision launch, the vote.  Beside it a gather ablation: the longest training set's problems for a fixed number of iterations (a
quarter of its rows, alternating labels, C = 10: no problem converges before) on the real Gram and on a copy whose row indices are
folded into its first 128 rows (the same reductions and barriers, gathers that stay in
the L2): the difference is what the far row gathers cost.
Host route: svm_cv(device=False) on the same Gram, timed once, if scikit-learn is importable where this runs; otherwise the record
says that no host time was taken on this machine.
usage: python tools/kernel_svm_bench.py [--steps K] [--warmup W] [--sizes 1000,3000] [--out profiles/kernel_svm_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import graph_kernel_oracle as O  # noqa: E402
from graph_kernel_bench import synthetic, timed  # noqa: E402
from kgcn_amd import graph_kernel as gk, ops  # noqa: E402


def cv_sets(G):
    trains, evals = [], []
    for tv, te in gk._kfold(G, 5):
        for a, b in gk._kfold(len(tv), 5):
            trains.append(tv[a])
            evals.append([tv[b], te])
    return trains, evals


def ablation(K, train):
    """µs an iteration of five problems on the longest training set, stopped at max_iter, on K and on a folded copy."""
    out = {}
    n = len(train)
    iters = n // 4
    sign = np.where(np.arange(n) % 2, 1, -1)
    for name, idx, mat in (("real_gram", train, K), ("folded_into_128_rows", train % 128, K[:128, :128].contiguous())):
        sets = ops.SvmSets([idx], [sign], graphs=int(mat.shape[0]))

        def run():
            try:
                return int(ops.svm_smo_batch(mat, sets, [0] * 5, [10.0] * 5, tol=1e-12, max_iter=iters, iters_per_launch=iters)[2].max().item())
            except ops.SvmNotConverged as e:
                return int(e.result[2].max().item())
        t, done = timed(run, 3, 1)
        out[name] = {"rows": n, "iterations": done, "ms": t["median_ms"], "us_per_iteration": t["median_ms"] * 1e3 / max(done, 1)}
    return out


def bench_set(name, K, y, steps, warmup, host):
    G = int(K.shape[0])
    C_grid = np.linspace(1e-4, 10, 5)
    trains, evals = cv_sets(G)
    rec = {"set": name, "graphs": G, "fits": len(trains) * len(C_grid), "training_rows": [int(min(map(len, trains))), int(max(map(len, trains)))],
           "tol": 1e-3, "iters_per_launch": ops.SVM_DEFAULT_SLICE}
    rec["device_svm_cv"], res = timed(lambda: gk.svm_cv(K, y, device=True), steps, warmup)
    rec["device_result"] = {k: res[k] for k in ("best_C", "val_acc", "test_acc", "mean", "std")}
    rec["smo"], batch = timed(lambda: gk.svm_fit(K, y, trains, C_grid), steps, warmup)
    it = batch.n_iter.cpu().numpy()
    rec["smo"].update(launches=batch.slices, iterations_longest=int(it.max()), iterations_all=int(it.sum()),
                      iterations_by_C=[int(it.reshape(len(trains), len(C_grid))[:, c].max()) for c in range(len(C_grid))],
                      us_per_iteration_longest=rec["smo"]["median_ms"] * 1e3 / max(int(it.max()), 1))
    rec["decision_and_vote"], _ = timed(lambda: gk.svm_predict(batch, K, evals, return_correct=True), steps, warmup)
    jobs = gk._svm_jobs(batch, K, evals)
    rec["decision"], _ = timed(lambda: gk._svm_jobs(batch, K, evals), steps, warmup)
    rec["vote"], _ = timed(lambda: ops.svm_vote(jobs[0], jobs[1], jobs[3], [g[3] for g in jobs[4]], [g[4] for g in jobs[4]], 2, batch.labels),
                           steps, warmup)
    rec["gather_ablation"] = ablation(K, max(trains, key=len)) if G >= 256 else None
    if host:
        Kh = K.cpu().numpy()
        t0 = time.perf_counter()
        ref = gk.svm_cv(Kh, y, device=False)
        rec["host_svm_cv_s"] = time.perf_counter() - t0
        rec["host_result"] = {k: ref[k] for k in ("best_C", "val_acc", "test_acc", "mean", "std")}
        rec["host_cpus"] = os.cpu_count()
    else:
        rec["host_svm_cv_s"] = None
        rec["host_note"] = "scikit-learn is not importable on this machine: no host time was taken here"
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sizes", default="1000,3000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kernel_svm_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "kernel_svm_bench needs the GPU"
    try:
        import sklearn
        host = sklearn.__version__
    except ImportError:
        host = None
    props = torch.cuda.get_device_properties(0)
    z = np.load(os.path.join(ROOT, "tests", "golden", "g13_graph_kernel.npz"), allow_pickle=False)
    sets = [("fixture", O.unpack_graphs(z, "two_"), z["two_y"])]
    for s in (int(s) for s in args.sizes.split(",") if s):
        graphs = synthetic(s)
        rare = np.array([int((g[2] >= 2).sum()) for g in graphs])
        sets.append(("synthetic_%d" % s, graphs, (rare > np.median(rare)).astype(np.int64)))
    out = {"device": props.name, "compute_units": props.multi_processor_count, "scikit_learn": host, "steps": args.steps,
           "warmup": args.warmup, "timing": "host clock between device synchronisations, ms", "sets": []}
    for name, graphs, y in sets:
        adjs, nn, lab = O.to_adjs(graphs)
        K = gk.wl_subtree_kernel(adjs, nn, lab, iterations=3)
        rec = bench_set(name, K, y, args.steps, args.warmup, host is not None)
        out["sets"].append(rec)
        print(json.dumps(rec), flush=True)
        with open(args.out, "w") as f:                                # kept after every set: a later set may not finish
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
