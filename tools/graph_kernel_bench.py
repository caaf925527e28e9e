#!/usr/bin/env python3
"""The classical graph kernels (kgcn_amd/graph_kernel.py, csrc/graphkern.hip) stage by stage, one JSON record per data set:
the two-class fixture of tests/golden/g13_graph_kernel.npz (120 graphs) and synthetic molecule-like sets of 50-node graphs
(a random tree with short branches plus ring closures, 5 skewed labels) at 3,000 and 20,000 graphs.

For the WL kernel (3 iterations) and the SP kernel: the wall time of every stage between device synchronisations (median,
minimum and maximum over --steps repeats after --warmup) -- refine, rank, runs, SP features, the Gram plan (column sort, diagonal
route), the dense Gram passes, the normalisation -- and of the whole public call including the host packing; the columns, the
share that took the diagonal route and the dense column count; the dense passes' share of the f64 MFMA peak (2 G_pad^2 / 2 flop a
dense column over the upper-triangle tiles: what the kernel executes, not what a sparse product would need).  Beside it the numpy
oracle of tests/graph_kernel_oracle.py on the same inputs (timed once, up to --oracle-max graphs) and whether the Grams are equal.
usage: python tools/graph_kernel_bench.py [--steps K] [--warmup W] [--sizes 3000,20000] [--oracle-max N] [--out profiles/graph_kernel_bench.json]"""
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
import graph_kernel_oracle as O  # noqa: E402
from kgcn_amd import graph_kernel as gk, ops  # noqa: E402

MFMA_F64_TFLOPS = 78.6


def synthetic(T, n=50, seed=0):
    rng = np.random.default_rng(seed)
    graphs = []
    for _ in range(T):
        parent = np.maximum(np.arange(1, n) - rng.integers(1, 4, n - 1), 0)
        pairs = np.stack([np.arange(1, n), parent], 1)
        a = rng.integers(6, n, 3)
        ring = np.stack([a, a - rng.integers(4, 7, 3)], 1)             # closes rings of 5 to 7 nodes or larger
        graphs.append((n, O.both_ways(np.concatenate([pairs, ring])), rng.choice(5, n, p=[0.6, 0.15, 0.15, 0.07, 0.03])))
    return graphs


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


def gram_stages(runs, G, steps, warmup, rec):
    col, graph, count = (torch.cat([r[i] for r in runs]) for i in range(3))
    rec["run_count"] = int(col.numel())
    # the two halves of ops.gram_from_runs, called as it calls them
    from kgcn_amd._lib import check, current_stream, lib, ptr, workspace
    n, cc = int(col.numel()), ops.GRAM_CHUNK_COLS
    wsb = lib.kgcn_graph_gram_workspace_bytes(n, G, cc)
    ws = workspace(wsb, col.device, torch.uint8)
    stats = torch.empty((3,), device=col.device, dtype=torch.int64)
    K = torch.empty((G, G), device=col.device, dtype=torch.float64)
    rec["gram_plan_and_diagonal"], _ = timed(lambda: check(lib.kgcn_gram_plan_i64(
        ptr(col), ptr(graph), ptr(count), n, G, cc, ptr(stats), ptr(ws), wsb, current_stream()), "plan"), steps, warmup)
    cols, diag, dense = stats.tolist()
    rec.update(columns=cols, diag_columns=diag, dense_columns=dense, diag_share=diag / max(cols, 1), chunk_cols=cc)
    rec["gram_dense"], _ = timed(lambda: check(lib.kgcn_gram_dense_f64(
        ptr(graph), ptr(count), n, G, dense, cc, ptr(K), ptr(ws), wsb, current_stream()), "dense"), steps, warmup)
    g_pad = -(-G // 64) * 64
    chunks = -(-dense // cc)
    flop = 2.0 * (g_pad * (g_pad + 64) / 2) * chunks * cc
    rec["gram_dense_executed_gflop"] = flop / 1e9
    rec["gram_dense_share_of_f64_mfma_peak"] = flop / (rec["gram_dense"]["median_ms"] * 1e-3) / (MFMA_F64_TFLOPS * 1e12) if dense else None
    rec["normalize"], _ = timed(lambda: ops.gram_normalize(K), steps, warmup)
    return K


def bench_set(name, graphs, steps, warmup, oracle):
    adjs, nn, lab = O.to_adjs(graphs)
    rec = {"set": name, "graphs": len(graphs), "padded_nodes": int(max(nn)), "nodes": int(nn.sum())}
    t0 = time.perf_counter()
    gs = gk.GraphSet(adjs, nn, lab)
    torch.cuda.synchronize()
    rec["host_packing_ms"] = (time.perf_counter() - t0) * 1e3
    rec["entries"] = gs.csr.nnz
    # ---- WL
    wl = {}
    col0, _ = gs.initial_colours("node")
    cols, refine, rank = [col0], [], []
    for it in range(3):
        t, (nbr, hi, lo) = timed(lambda: ops.wl_refine(gs.csr, gs.num_nodes, cols[-1]), steps, warmup)
        refine.append(t)
        t, (new, info) = timed(lambda: ops.wl_rank(gs.csr, gs.num_nodes, cols[-1], nbr, hi, lo), steps, warmup)
        rank.append(t)
        assert int(info[1].item()) == 0
        wl.setdefault("colours", []).append(int(info[0].item()))
        cols.append(new)
    wl["refine"], wl["rank"] = refine, rank
    wl["runs"], runs = timed(lambda: [ops.wl_runs(c, gs.num_nodes, gs.T, gs.M, it << 32) for it, c in enumerate(cols)], steps, warmup)
    K_wl = gram_stages(runs, gs.T, steps, warmup, wl)
    wl["whole_call"], K2 = timed(lambda: gk.wl_subtree_kernel(adjs, nn, lab, normalize=False), steps, warmup)
    wl["whole_call_on_packed_set"], _ = timed(lambda: gk.wl_subtree_kernel(gs, normalize=False), steps, warmup)
    assert torch.equal(K2, K_wl)
    rec["wl"] = wl
    # ---- SP
    sp = {}
    col0, count = gs.initial_colours("node")
    sp["features"], runs = timed(lambda: ops.sp_features(gs.csr, gs.num_nodes, col0, count), steps, warmup)
    K_sp = gram_stages([runs], gs.T, steps, warmup, sp)
    sp["whole_call"], K2 = timed(lambda: gk.shortest_path_kernel(adjs, nn, lab, normalize=False), steps, warmup)
    sp["whole_call_on_packed_set"], _ = timed(lambda: gk.shortest_path_kernel(gs, normalize=False), steps, warmup)
    assert torch.equal(K2, K_sp)
    rec["sp"] = sp
    if oracle:
        t0 = time.perf_counter()
        ref = O.wl_gram(graphs, 3)
        rec["oracle_wl_s"] = time.perf_counter() - t0
        rec["oracle_wl_equal"] = bool(np.array_equal(K_wl.cpu().numpy(), ref.astype(np.float64)))
        t0 = time.perf_counter()
        ref = O.sp_gram(graphs)
        rec["oracle_sp_s"] = time.perf_counter() - t0
        rec["oracle_sp_equal"] = bool(np.array_equal(K_sp.cpu().numpy(), ref.astype(np.float64)))
    else:
        rec["oracle_wl_s"] = rec["oracle_sp_s"] = None
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="3000,20000")
    ap.add_argument("--oracle-max", type=int, default=3000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_kernel_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "graph_kernel_bench needs the GPU"
    props = torch.cuda.get_device_properties(0)
    z = np.load(os.path.join(ROOT, "tests", "golden", "g13_graph_kernel.npz"), allow_pickle=False)
    sets = [("fixture", O.unpack_graphs(z, "two_"))]
    sets += [("synthetic_%d" % int(s), synthetic(int(s))) for s in args.sizes.split(",") if s]
    import bench                                                      # its sensor reader: the clocks of the box, read only
    sensors = bench.BoxSensors(0)
    out = {"device": props.name, "compute_units": props.multi_processor_count, "sensors": sensors.source or sensors.why,
           "steps": args.steps, "warmup": args.warmup, "timing": "host clock between device synchronisations, ms",
           "sets": []}
    for name, graphs in sets:
        rec = bench_set(name, graphs, args.steps, args.warmup, len(graphs) <= args.oracle_max)
        rec["box_after"] = sensors.read() if sensors.source else None  # sclk / mclk / power right after the set's last kernels
        out["sets"].append(rec)
        print(json.dumps(rec), flush=True)
        with open(args.out, "w") as f:                                # kept after every set: a later set may not finish
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
