#!/usr/bin/env python3
"""Active learning on the device (kgcn_amd/active_learning.py over csrc/labelprop.hip) against scikit-learn on the host of the same
machine, one JSON record per size: n points in all (a tenth of them training rows, the rest the pool) of d = 512 fingerprint-like
bits drawn around 8 cluster prototypes, T = 4 two-class tasks, LabelSpreading(alpha = 0.2, tol = 1e-3), strategy "E".  gamma = 1 / d
on the standardised points: the reference's default gamma = 20 leaves no two of these points connected.

Per size:
  query              one ActiveLearner.query: standardise, affinity, degrees, propagate 4 tasks, score the pool, pick
  loop_reuse         query_and_teach_n_times(50, reuse=True): the union and its matrix built once
  loop_rebuild       query_and_teach_n_times(50, reuse=False): everything rebuilt per iteration in the reference's row order
  host               the same with scikit-learn (StandardScaler, one LabelSpreading per task refitted per iteration, scipy's entropy):
                     one query, and the loop for --host-iterations iterations (fewer at the large sizes: the record gives the
                     iterations timed, the seconds they took and the seconds per iteration; nothing is extrapolated silently)
  step               the propagation step alone: (time of 40 steps - time of 8 steps) / 32 with tol = 0, its n^2 * 8 bytes of W as a
                     fraction of the 8 TB/s HBM peak and of what kgcn_hbm_probe (read-only stream, 1 GiB) delivers in this run
Wall times between device synchronisations; median of --steps repeats after --warmup.
usage: python tools/active_learning_bench.py [--sizes 1000,5000,20000] [--steps 3] [--warmup 1] [--no-host] [--out FILE]"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kgcn_amd import _lib, active_learning as al, ops  # noqa: E402

D, TASKS, ROUNDS, ALPHA, TOL = 512, 4, 50, 0.2, 1e-3
HBM_PEAK = 8.0e12


def timed(fn, steps, warmup):
    for _ in range(warmup):
        out = fn()
    ts = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}, out


def synthetic(n, seed=0):
    rng = np.random.default_rng(seed)
    proto = rng.random((8, D)) < 0.15
    cluster = rng.integers(0, 8, n)
    X = (proto[cluster] ^ (rng.random((n, D)) < 0.05)).astype(np.float64)
    Y = np.stack([(cluster >> t) & 1 if t < 3 else (cluster % 3 == 0) for t in range(TASKS)], axis=1).astype(np.int64)
    Y = np.where(rng.random((n, TASKS)) < 0.05, 1 - Y, Y)
    Y[:2] = [[0] * TASKS, [1] * TASKS]                          # both classes of every task among the training rows
    m = max(n // 10, 2)
    return X[:m], Y[:m], X[m:], Y[m:]


def learner(Xt, Yt):
    return al.ActiveLearner(al.LabelSpreading(gamma=1.0 / D, alpha=ALPHA, tol=TOL), Xt, Yt, query_strategy="E")


def host_query(Xt, Yt, Xp):
    from scipy import stats
    from sklearn.preprocessing import StandardScaler
    from sklearn.semi_supervised import LabelSpreading
    X = StandardScaler().fit_transform(np.vstack([Xt, Xp]))
    Y = np.vstack([Yt, np.full((len(Xp), TASKS), -1)])
    ent = np.zeros(len(Xp))
    for t in range(TASKS):
        m = LabelSpreading(kernel="rbf", gamma=1.0 / D, alpha=ALPHA, tol=TOL).fit(X, Y[:, t])
        ent = ent + stats.entropy(m.label_distributions_[len(Xt):].T)
    return int(np.argsort(ent, kind="stable")[-1])


def host_loop(Xt, Yt, Xp, Yp, rounds):
    left, picked = list(range(len(Xp))), []
    for _ in range(rounds):
        p = host_query(Xt, Yt, Xp)
        Xt, Yt = np.vstack([Xt, Xp[p]]), np.vstack([Yt, Yp[p]])
        Xp, Yp = np.delete(Xp, p, axis=0), np.delete(Yp, p, axis=0)
        picked.append(left.pop(p))
    return picked


def step_alone(n, Xt, Xp, steps, warmup):
    X = ops.attr_scale(torch.from_numpy(np.vstack([Xt, Xp])).cuda())[0]
    W = ops.rbf_affinity(X, 1.0 / D)
    s, d = ops.lp_degrees(W)
    labels = torch.full((n, TASKS), -1, dtype=torch.int32)
    labels[:len(Xt)] = torch.arange(len(Xt), dtype=torch.int32)[:, None] % 2
    labels = labels.cuda()
    task_col = np.arange(TASKS + 1) * 2
    out = {}
    for name, variant, scale in (("spreading", ops.LP_SPREADING, d), ("propagation", ops.LP_PROPAGATION, s)):
        t = {m: timed(lambda: ops.lp_propagate(W, scale, labels, task_col, variant, alpha=ALPHA, tol=0.0, max_iter=m, iters_per_check=m),
                      steps, warmup)[0]["median_ms"] for m in (8, 40)}
        per = (t[40] - t[8]) / 32.0
        out[name] = {"ms_8_steps": t[8], "ms_40_steps": t[40], "ms_per_step": per, "bytes_of_W": n * n * 8,
                     "fraction_of_hbm_peak": n * n * 8 / (per * 1e-3) / HBM_PEAK}
    return out


def hbm_read_rate():
    nbytes = 1 << 30
    a = torch.zeros(nbytes // 4, device="cuda", dtype=torch.float32)
    b = torch.zeros(16, device="cuda", dtype=torch.float32)
    t, _ = timed(lambda: _lib.check(_lib.lib.kgcn_hbm_probe(2, _lib.ptr(a), None, _lib.ptr(b), nbytes, _lib.current_stream()),
                                    "kgcn_hbm_probe"), 5, 2)
    return nbytes / (t["median_ms"] * 1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,5000,20000")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-iterations", default="50,5,1", help="loop iterations timed on the host, per size")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "active_learning_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "active_learning_bench needs the GPU"
    warnings.simplefilter("ignore")
    try:
        import sklearn
        host = None if args.no_host else sklearn.__version__
    except ImportError:
        host = None
    props = torch.cuda.get_device_properties(0)
    probe = hbm_read_rate()
    out = {"device": props.name, "compute_units": props.multi_processor_count, "scikit_learn": host, "host_cpus": os.cpu_count(),
           "host_threads": os.environ.get("OMP_NUM_THREADS"), "d": D, "tasks": TASKS, "rounds": ROUNDS, "gamma": 1.0 / D,
           "estimator": "LabelSpreading(alpha=0.2, tol=1e-3)", "strategy": "E", "hbm_probe_read_bytes_per_s": probe,
           "timing": "host clock between device synchronisations, ms (host route: s)", "sizes": []}
    sizes = [int(s) for s in args.sizes.split(",") if s]
    host_iters = [int(s) for s in args.host_iterations.split(",")]
    for k, n in enumerate(sizes):
        Xt, Yt, Xp, Yp = synthetic(n)
        rec = {"n": n, "training_rows": len(Xt), "pool_rows": len(Xp)}
        rec["query"], first = timed(lambda: learner(Xt, Yt).query(Xp)[0], args.steps, args.warmup)
        rec["loop_reuse"], reuse = timed(lambda: learner(Xt, Yt).query_and_teach_n_times(ROUNDS, Xp, Yp, reuse=True), args.steps, args.warmup)
        rec["loop_rebuild"], rebuild = timed(lambda: learner(Xt, Yt).query_and_teach_n_times(ROUNDS, Xp, Yp, reuse=False), 1, 0)
        probe_learner = learner(Xt, Yt)
        probe_learner.query(Xp)
        rec["n_iter_first_query"] = [int(v) for v in probe_learner.n_iter_history_[0]]
        rec["picks_equal_reuse_rebuild"] = reuse == rebuild
        rec["first_pick"] = int(first)
        rec["step"] = step_alone(n, Xt, Xp, args.steps, args.warmup)
        for v in rec["step"].values():
            v["fraction_of_hbm_probe"] = v["bytes_of_W"] / (v["ms_per_step"] * 1e-3) / probe
        if host:
            it = host_iters[min(k, len(host_iters) - 1)]
            t0 = time.perf_counter()
            hp = host_query(Xt, Yt, Xp)
            t1 = time.perf_counter()
            hl = host_loop(Xt, Yt, Xp, Yp, it)
            t2 = time.perf_counter()
            rec["host"] = {"query_s": t1 - t0, "loop_iterations_timed": it, "loop_s": t2 - t1, "loop_s_per_iteration": (t2 - t1) / it,
                           "first_pick": hp, "picks_equal_device": hl == reuse[:it]}
        else:
            rec["host"] = None
        out["sizes"].append(rec)
        print(json.dumps(rec), flush=True)
        with open(args.out, "w") as f:                              # kept after every size: a later size may not finish
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
