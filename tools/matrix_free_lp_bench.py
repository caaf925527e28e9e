#!/usr/bin/env python3
"""The label-propagation step on a stored affinity matrix (ops.lp_propagate: a stream over n^2 * 8 bytes) against the matrix-free
step (ops.lp_propagate_free: every 64 x 64 tile of W rebuilt on the fp64 matrix pipe where it is consumed), and predict_proba
through ops.rbf_apply.  Writes profiles/matrix_free_lp_bench.json.

  steps      n = 1,000 / 5,000 / 20,000 standard-normal points of d = 8 and d = 512 attributes, gamma = 1 / d, 4 two-class tasks
             (8 columns), spreading and propagation: the time of one step = (time of 40 steps - time of 8 steps) / 32 with tol = 0,
             both routes in the same run; the results of the two routes are compared bit for bit on the way
  large      the matrix-free step alone at n = 100,000 (W would take 80 GB) and d = 8, from (12 steps - 4 steps) / 8 (--large-dims
             8,512 adds d = 512: about 1.5 s a step, a quarter of an hour in all)
  predict    LabelSpreading.predict_proba of 100,000 queries against 20,000 fitted points, d = 8 and d = 512, two classes
Host clock between device synchronisations; median, smallest and largest of --steps repeats (at least 10) after --warmup.
--resume FILE takes the records FILE already holds (an earlier run of this tool that did not finish) and measures only the others.
usage: python tools/matrix_free_lp_bench.py [--sizes 1000,5000,20000] [--dims 8,512] [--large 100000] [--large-dims 8] [--steps 10]
                                            [--warmup 2] [--resume FILE] [--out FILE]"""
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
from kgcn_amd import active_learning as al, ops  # noqa: E402

TASKS, ALPHA = 4, 0.2


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
    return np.array(ts), out


def per_step(run, few, many, steps, warmup):
    """-> median / min / max of (time of `many` steps - median time of `few` steps) / (many - few), ms."""
    base = float(np.median(timed(lambda: run(few), steps, warmup)[0]))
    ts, out = timed(lambda: run(many), steps, warmup)
    per = (ts - base) / (many - few)
    return {"median_ms": float(np.median(per)), "min_ms": float(per.min()), "max_ms": float(per.max()), "steps": [few, many]}, out


def problem(n, d, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    X = torch.randn((n, d), generator=g, dtype=torch.float64).cuda()
    labels = torch.full((n, TASKS), -1, dtype=torch.int32)
    m = max(n // 10, 2)
    labels[:m] = torch.arange(m, dtype=torch.int32)[:, None] % 2
    return X, labels.cuda(), np.arange(TASKS + 1) * 2


def routes(X, gamma, labels, task_col, stored, steps, warmup, few=8, many=40):
    rec = {}
    sd_free = ops.rbf_degrees(X, gamma)
    if stored:
        W = ops.rbf_affinity(X, gamma)
        sd = ops.lp_degrees(W)
        rec["degrees_equal_bits"] = bool(torch.equal(sd[0], sd_free[0]) and torch.equal(sd[1], sd_free[1]))
    for name, variant, k in (("spreading", ops.LP_SPREADING, 1), ("propagation", ops.LP_PROPAGATION, 0)):
        kw = dict(alpha=ALPHA, tol=0.0)
        r = {}
        r["matrix_free"], free = per_step(lambda m: ops.lp_propagate_free(X, gamma, sd_free[k], labels, task_col, variant, max_iter=m,
                                                                          iters_per_check=m, **kw)[0], few, many, steps, warmup)
        if stored:
            r["stored"], kept = per_step(lambda m: ops.lp_propagate(W, sd[k], labels, task_col, variant, max_iter=m, iters_per_check=m,
                                                                    **kw)[0], few, many, steps, warmup)
            r["equal_bits"] = bool(torch.equal(free, kept))
            r["matrix_free_over_stored"] = r["matrix_free"]["median_ms"] / r["stored"]["median_ms"]
            r["faster"] = "matrix_free" if r["matrix_free_over_stored"] < 1.0 else "stored"
        rec[name] = r
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,5000,20000")
    ap.add_argument("--dims", default="8,512")
    ap.add_argument("--large", type=int, default=100000)
    ap.add_argument("--large-dims", default="8")
    ap.add_argument("--resume", default=None)
    ap.add_argument("--queries", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matrix_free_lp_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "matrix_free_lp_bench needs the GPU"
    warnings.simplefilter("ignore")
    props = torch.cuda.get_device_properties(0)
    out = {"device": props.name, "compute_units": props.multi_processor_count, "tasks": TASKS, "columns": 2 * TASKS, "gamma": "1 / d",
           "timing": "host clock between device synchronisations, ms; per step = (t(many steps) - median t(few steps)) / (many - few)",
           "repeats": args.steps, "steps": [], "large": [], "predict": []}
    if args.resume:
        with open(args.resume) as f:
            out.update({k: v for k, v in json.load(f).items() if k in ("steps", "large", "predict")})

    def have(section, n, d):
        return any(r["n"] == n and r["d"] == d for r in out[section])

    def keep():
        with open(args.out, "w") as f:                              # kept after every record: a later one may not finish
            json.dump(out, f, indent=1)
            f.write("\n")
    dims = [int(s) for s in args.dims.split(",") if s]
    for d in dims:
        for n in [int(s) for s in args.sizes.split(",") if s]:
            if have("steps", n, d):
                continue
            X, labels, task_col = problem(n, d)
            rec = {"n": n, "d": d, "bytes_of_W": n * n * 8}
            rec.update(routes(X, 1.0 / d, labels, task_col, True, args.steps, args.warmup))
            out["steps"].append(rec)
            print(json.dumps(rec), flush=True)
            keep()
    for d in [int(s) for s in args.large_dims.split(",") if s] if args.large else ():
        if have("large", args.large, d):
            continue
        X, labels, task_col = problem(args.large, d)
        rec = {"n": args.large, "d": d, "bytes_of_W": args.large * args.large * 8}
        rec.update(routes(X, 1.0 / d, labels, task_col, False, args.steps, 1, few=4, many=12))
        out["large"].append(rec)
        print(json.dumps(rec), flush=True)
        keep()
    for d in dims if args.queries else ():
        n = 20000
        if have("predict", n, d):
            continue
        X, labels, _ = problem(n, d)
        est = al.LabelSpreading(gamma=1.0 / d, alpha=ALPHA, max_iter=30)
        est.matrix_free = True
        est.fit(X, labels[:, 0].cpu().numpy())
        Xq = torch.randn((args.queries, d), generator=torch.Generator(device="cpu").manual_seed(1), dtype=torch.float64).cuda()
        ts, proba = timed(lambda: est.predict_proba(Xq), args.steps, args.warmup)
        ta, _ = timed(lambda: ops.rbf_apply(Xq, est.X_, 1.0 / d, est._dist), args.steps, args.warmup)
        rec = {"queries": args.queries, "n": n, "d": d, "classes": int(proba.shape[1]), "bytes_of_the_kernel": args.queries * n * 8,
               "predict_proba": {"median_ms": float(np.median(ts)), "min_ms": float(ts.min()), "max_ms": float(ts.max())},
               "rbf_apply_alone": {"median_ms": float(np.median(ta)), "min_ms": float(ta.min()), "max_ms": float(ta.max())},
               "nan_rows": int(np.isnan(proba).any(axis=1).sum())}
        out["predict"].append(rec)
        print(json.dumps(rec), flush=True)
        keep()


if __name__ == "__main__":
    main()
