#!/usr/bin/env python3
"""Integrated gradients of the compound-protein interaction multitask network at the reference's size: N = 50 nodes, F = 81
features, T = 4 tasks, D = 100 steps (101 copies), modal 'all', for 1 and for 256 compounds.

  fused     visualization.cpi_integrated_gradients: P, Q, Y0 once per compound, ops.cpi_ig (csrc/cpiig.hip) over the copies, one
            GraphConv backward per (compound, task).  Wall time of the whole call, and of the sweep's three kernels alone.
  composed  fused=False: the 101 copies as batch rows through the model, one autograd backward per task.
  loop      the generic visualization.integrated_gradients: one forward and one backward per step, per compound and task
            (D T GraphConv(512) passes a compound), on --loop-compounds compounds.

Every timing is a host clock around work that ends in a device synchronise, after a warm-up of the same shapes, the median of
--repeats runs.  Prints one JSON line; --out writes it to a file as well.  There is no threshold: the expectation is only that
the composed route does (D + 1) times the GEMM work of the fused one.

    python tools/cpi_ig_bench.py [--repeats 5] [--loop-compounds 2] [--out profiles/cpi_ig_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kgcn_amd import data_util as D, models, ops, visualization as V  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--loop-compounds", type=int, default=2)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda:0")
N, F, T, G, STEPS = 50, 81, 4, 256, args.steps
rng = np.random.default_rng(0)
dense = np.zeros((G, N, N), np.float32)
x = np.zeros((G, N, F), np.float32)
for g in range(G):                                           # molecule-like graphs: self loops and about three bonds a node
    m = int(rng.integers(20, N + 1))
    x[g, :m] = rng.standard_normal((m, F))
    for i in range(m):
        dense[g, i, i] = 1.0
        for j in rng.integers(0, m, size=3):
            dense[g, i, j] = dense[g, j, i] = 1.0
dataset = D.DeviceGraphDataset([D.FlatAdjacency.from_dense(dense)], x, device=dev)
torch.manual_seed(0)
model = models.CPIMultitaskNet(1, T).to(dev)
with torch.no_grad():
    adj, xb = dataset.batch(np.arange(4))
    model(xb, adj)
    model.out.kernel.mul_(2.0 / N)                           # predictions away from saturation


def median_time(fn, repeats):
    fn()                                                     # warm-up of the same shapes
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), [round(t, 5) for t in ts]


def sweep_alone(C):
    """The three kernels of ops.cpi_ig on random P, Q of C compounds."""
    co = V.cpi_ig_coefficients("all", "ig", STEPS)
    P = torch.randn((C, N, 512), device=dev)
    Q = torch.randn((C, N, 512), device=dev) * 0.2
    u = torch.randn((T, 512), device=dev) * (2.0 / (N * 512 ** 0.5))
    e = torch.zeros(T, device=dev)
    al, ga, wA, wB = (torch.tensor(co[k], device=dev, dtype=torch.float32) for k in ("alpha", "gamma", "wA", "wB"))
    return median_time(lambda: ops.cpi_ig(P, Q, u, e, al, ga, wA, wB), args.repeats)


def loop_route(cids):
    """The generic per-step loop for every task of the compounds `cids`."""
    out = []
    for cid in cids:
        adj1, x1 = dataset.batch([cid])
        for t in range(T):
            score = lambda f, a, t=t: torch.softmax(model(f, a), dim=1)[0, 1, t]
            out.append(V.integrated_gradients(score, x1, adj1, divide_number=STEPS))
    return out


result = {"nodes": N, "features": F, "tasks": T, "steps": STEPS, "width": 512, "modal": "all", "repeats": args.repeats,
          "device": torch.cuda.get_device_name(0)}
for p in model.parameters():
    p.requires_grad_(False)
for C in (1, G):
    ids = list(range(C))
    kw = dict(divide_number=STEPS, modal="all", compounds=ids)
    t_fused, all_fused = median_time(lambda: V.cpi_integrated_gradients(model, None, dataset, **kw), args.repeats)
    t_comp, all_comp = median_time(lambda: V.cpi_integrated_gradients(model, None, dataset, fused=False, **kw), args.repeats)
    t_sweep, _ = sweep_alone(C)
    result["compounds_%d" % C] = {"fused_wall_s": round(t_fused, 5), "fused_runs_s": all_fused, "fused_sweep_kernels_s": round(t_sweep, 6),
                                  "composed_wall_s": round(t_comp, 5), "composed_runs_s": all_comp,
                                  "composed_over_fused": round(t_comp / t_fused, 2),
                                  "fused_ms_per_compound": round(1e3 * t_fused / C, 4),
                                  "composed_ms_per_compound": round(1e3 * t_comp / C, 4)}
nl = max(1, min(args.loop_compounds, G))
t_loop, all_loop = median_time(lambda: loop_route(range(nl)), max(1, min(args.repeats, 3)))
result["loop"] = {"compounds": nl, "wall_s": round(t_loop, 4), "runs_s": all_loop, "ms_per_compound": round(1e3 * t_loop / nl, 2)}
# the three routes agree (max abs difference of features_IG over max abs value, compound 0)
fused = V.cpi_integrated_gradients(model, None, dataset, divide_number=STEPS, modal="all", compounds=[0])
comp = V.cpi_integrated_gradients(model, None, dataset, divide_number=STEPS, modal="all", compounds=[0], fused=False)
loop = loop_route([0])
big = max(float(np.abs(r["features_IG"]).max()) for r in fused)
result["features_IG_max_rel_diff_fused_vs_composed"] = max(float(np.abs(a["features_IG"] - b["features_IG"]).max()) for a, b in zip(fused, comp)) / big
result["features_IG_max_rel_diff_fused_vs_loop"] = max(float(np.abs(a["features_IG"] - b["features"][0].cpu().numpy()).max())
                                                       for a, b in zip(fused, loop)) / big
line = json.dumps(result)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
