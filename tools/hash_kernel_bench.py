#!/usr/bin/env python3
"""The hash graph kernels (kgcn_amd.graph_kernel.hash_graph_kernel, csrc/hashkern.hip and the copies route of csrc/graphkern.hip)
stage by stage, one JSON record per data set: the synthetic molecule-like sets of tools/graph_kernel_bench.py (50-node graphs) at
--sizes graphs with d = --dim attributes a node correlated with the node label, R = --draws projections.

Per base kernel (WL with 3 refinements, SP), labels=None: the wall time of every stage of the batched route between device
synchronisations (median, minimum, maximum over --steps repeats after --warmup) -- scale, buckets, the (draw, bucket) rank, every
refinement (refine + rank over all draws, with its one mismatch read-back), the runs, the Gram plan / dense passes / normalisation
-- then the whole public call on a packed GraphSet with batched=True against batched=False (the R draws one after another through
wl_colourings, ops.wl_runs, ops.sp_features: the code the classical kernels already had), alternating, with whether their Grams
are bit-equal, and the Gram's share of the batched call.  The numpy oracle of tests/hash_kernel_oracle.py is timed once on the
first --oracle-max graphs and compared with the device on the same graphs.
--bases picks the base kernels of a run and --append adds its sets to an existing file: the 20,000-graph set is run for WL alone
with one timed repeat (SP's n^2 keys a draw and graph give it 20 times the runs of WL, and every dense Gram pass costs 44 times
the 3,000-graph one).
usage: python tools/hash_kernel_bench.py [--steps K] [--warmup W] [--sizes 100,3000] [--bases wl,sp] [--dim 64] [--draws 20]
                                         [--oracle-max N] [--append] [--out profiles/hash_kernel_bench.json]"""
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
import hash_kernel_oracle as H  # noqa: E402
from graph_kernel_bench import gram_stages, synthetic, timed  # noqa: E402
from kgcn_amd import graph_kernel as gk, ops  # noqa: E402


def attributes(graphs, d, seed=1):
    """[Nv, d]: a label-dependent shift of every column plus unit noise."""
    rng = np.random.default_rng(seed)
    lab = np.concatenate([np.asarray(g[2])[:g[0]] for g in graphs])
    shift = rng.standard_normal((5, d)) * 1.5
    return shift[lab] + rng.standard_normal((len(lab), d))


def alternating(fa, fb, steps, warmup):
    """Two versions timed in turn in the same window -> (stats a, stats b, last results)."""
    for _ in range(warmup):
        ra, rb = fa(), fb()
    ta, tb = [], []
    for _ in range(steps):
        for fn, ts in ((fa, ta), (fb, tb)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
            if fn is fa:
                ra = out
            else:
                rb = out
    stat = lambda ts: {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}  # noqa: E731
    return stat(ta), stat(tb), ra, rb


def bench_set(name, graphs, d, R, steps, warmup, oracle_max, bases):
    adjs, nn, lab = O.to_adjs(graphs)
    X = attributes(graphs, d)
    attrs = H.to_attributes(graphs, X)
    V, b = gk.lsh_draws(0, R, d)
    gs = gk.GraphSet(adjs, nn, lab)
    T, M, dev = gs.T, gs.M, gs.device
    rec = {"set": name, "graphs": T, "padded_nodes": M, "nodes": int(nn.sum()), "entries": gs.csr.nnz, "dim": d, "draws": R,
           "steps": steps, "warmup": warmup}
    x = torch.from_numpy(X).to(dev)
    Vd, bd = torch.from_numpy(V).to(dev), torch.from_numpy(b).to(dev)
    rec["scale"], (xs, _, _) = timed(lambda: ops.attr_scale(x), steps, warmup)
    rec["buckets"], bucket = timed(lambda: ops.lsh_buckets(xs, Vd, bd, 1.0), steps, warmup)
    exists = torch.from_numpy(gs.exists.reshape(-1)).to(dev)
    markR = (exists.to(torch.int32) - 1).repeat(R)
    full = torch.zeros((R, T * M), device=dev, dtype=torch.int64)
    full[:, exists] = bucket
    draw = torch.arange(R, device=dev, dtype=torch.int64)[:, None].expand(R, T * M).reshape(-1).contiguous()
    rec["rank_draw_bucket"], (col0, info) = timed(lambda: ops.rank_pairs(draw, full.reshape(-1), markR), steps, warmup)
    rec["hash_classes_all_draws"] = int(info[0].item())
    for base in bases:
        one = {}
        if base == "wl":
            cols, one["refinements"], one["colours"] = [col0], [], []
            for it in range(3):
                def refinement():
                    nbr, hi, lo = ops.wl_refine_copies(gs.csr, gs.num_nodes, cols[-1], R)
                    new, info = ops.wl_rank_copies(gs.csr, gs.num_nodes, cols[-1], R, nbr, hi, lo)
                    assert int(info[1].item()) == 0
                    return new, int(info[0].item())
                t, (new, count) = timed(refinement, steps, warmup)
                one["refinements"].append(t)
                one["colours"].append(count)
                cols.append(new)
            one["runs"], runs = timed(lambda: [ops.wl_runs_copies(c, gs.num_nodes, T, M, R, it << 32, 4 << 32) for it, c in enumerate(cols)],
                                      steps, warmup)
        else:
            c = col0.view(R, T * M)
            first = torch.where(c >= 0, c, torch.full_like(c, 2 ** 31 - 1)).amin(dim=1, keepdim=True)
            c = torch.where(c >= 0, c - first, c).contiguous()
            count = int(c.max().item()) + 1
            one["classes_per_draw_max"] = count
            one["runs"], r1 = timed(lambda: ops.sp_features_copies(gs.csr, gs.num_nodes, c.reshape(-1), R, count), steps, warmup)
            runs = [r1]
        gram_stages(runs, T, steps, warmup, one)
        kw = dict(attributes=attrs, base=base, projections=V, offsets=b, normalize=True)
        one["whole_call_batched"], one["whole_call_per_draw"], Ka, Kb = alternating(
            lambda: gk.hash_graph_kernel(gs, batched=True, **kw), lambda: gk.hash_graph_kernel(gs, batched=False, **kw), steps, warmup)
        one["routes_bit_equal"] = bool(torch.equal(Ka, Kb))
        one["batched_over_per_draw"] = one["whole_call_batched"]["median_ms"] / one["whole_call_per_draw"]["median_ms"]
        gram_ms = one["gram_plan_and_diagonal"]["median_ms"] + one["gram_dense"]["median_ms"] + one["normalize"]["median_ms"]
        one["gram_share_of_batched_call"] = gram_ms / one["whole_call_batched"]["median_ms"]
        rec[base] = one
    n = min(T, oracle_max)
    if n:
        sub = graphs[:n]
        rows = int(sum(g[0] for g in sub))
        adjs_s, nn_s, lab_s = O.to_adjs(sub, M)
        for base in bases:
            t0 = time.perf_counter()
            ref = H.hash_gram(sub, X[:rows], V, b, 1.0, base, 3, None, normalize=True)
            rec["oracle_%s_s" % base] = time.perf_counter() - t0
            got = gk.hash_graph_kernel(adjs_s, nn_s, attrs[:n], base=base, projections=V, offsets=b).cpu().numpy()
            rec["oracle_%s_equal" % base] = bool(np.array_equal(got.view(np.uint64), ref.view(np.uint64)))
        rec["oracle_graphs"] = n
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="100,3000")
    ap.add_argument("--bases", default="wl,sp")
    ap.add_argument("--append", action="store_true", help="add the sets to the file --out already holds")
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--draws", type=int, default=20)
    ap.add_argument("--oracle-max", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hash_kernel_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "hash_kernel_bench needs the GPU"
    props = torch.cuda.get_device_properties(0)
    out = {"device": props.name, "compute_units": props.multi_processor_count,
           "timing": "host clock between device synchronisations, ms; the two routes of a whole call alternate in one window",
           "sets": []}
    if args.append:
        with open(args.out) as f:
            out = json.load(f)
    for s in [int(s) for s in args.sizes.split(",") if s]:
        rec = bench_set("synthetic_%d" % s, synthetic(s), args.dim, args.draws, args.steps, args.warmup, args.oracle_max,
                        [b for b in args.bases.split(",") if b])
        out["sets"].append(rec)
        print(json.dumps(rec), flush=True)
        with open(args.out, "w") as f:                                # kept after every set: a later set may not finish
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
