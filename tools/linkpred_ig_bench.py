#!/usr/bin/env python3
"""Integrated gradients of the link-prediction gcn at the size of tests/golden/g8_kg_linkpred.npz (N = 5,000, 44,920 adjacency
entries): the fused path against the composed one.

  fused     visualization.linkpred_integrated_gradients over the WHOLE test label list (9,980 targets, edge_score, 30 steps,
            reduce='node'): the stash once, then ops.kg_ig (csrc/kgig.hip) in chunks.  Wall time, and the kernel launches alone.
  composed  what the parent commit offers: per target and step the model's two GraphConv layers on the scaled table and
            torch.autograd.grad back to it (30 forward + backward passes a target), on --sample targets.

Prints one JSON line.  The claim to check is only fused per-target time < composed per-target time.

    python tools/linkpred_ig_bench.py [--sample 20] [--targets 9980]
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
ap.add_argument("--sample", type=int, default=20)
ap.add_argument("--targets", type=int, default=None)
ap.add_argument("--steps", type=int, default=30)
args = ap.parse_args()

dev = torch.device("cuda:0")
z = np.load(os.path.join(ROOT, "tests", "golden", "g8_kg_linkpred.npz"))
data = D.LinkPredictionData({"adj": [(z["adj_idx"], z["adj_val"], np.array([int(z["node_num"])] * 2))], "node": z["node"],
                             "node_num": z["node_num"], "label_list": z["label_list"], "test_label_list": z["test_label_list"]})
adj = data.adjacency(dev)
labels = data.test_label_list[:args.targets] if args.targets else data.test_label_list
torch.manual_seed(0)
model = models.LinkPredictionNet("gcn", data.num_nodes, data.num_relations, seed=1234, device=dev)
with torch.no_grad():
    model.node_rows(adj)
N, K = data.num_nodes, args.steps


def sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


# ---- fused ---------------------------------------------------------------------------------------------------------------
V.linkpred_integrated_gradients(model, adj, labels, "edge_score", target=list(range(4)), divide_number=K)      # warm-up
t_fused, res = sync_time(lambda: V.linkpred_integrated_gradients(model, adj, labels, "edge_score", divide_number=K))
scales, weights = V.ig_scales("ig", K)
t_stash, st = sync_time(lambda: V.linkpred_ig_stash(model, adj, scales))
tg = np.concatenate([labels[:, [0, 2]], np.full((len(labels), 2), -1)], 1).astype(np.int32)
run = lambda: ops.kg_ig(adj.channels[0], st["g1"], st["rowsum"], st["b1"], st["w2"], st["h2"], st["p"], scales, weights, tg)
run()
t_kernel, _ = sync_time(run)

# ---- composed --------------------------------------------------------------------------------------------------------------
E = model.embedding.detach()
for p in model.parameters():
    p.requires_grad_(False)


def composed(row):
    a, b = int(row[0]), int(row[2])
    ig = torch.zeros_like(E)
    for k in range(K):
        x = (E * ((k + 1) / float(K))).view(1, N, -1).requires_grad_(True)
        h = model.conv2(model.conv1(x, adj=adj), adj=adj).view(N, -1)
        g, = torch.autograd.grad((h[a] * h[b]).sum(), x)
        ig += g.view(N, -1) * E / float(K)
    return ig


composed(labels[0])
sample = labels[:args.sample]
t_comp, igs = sync_time(lambda: [composed(r) for r in sample])
agree = max(float(np.abs(ig.sum(-1).cpu().numpy() - r["node_ig"]).max() / max(np.abs(r["node_ig"]).max(), 1e-30))
            for ig, r in zip(igs, res))
print(json.dumps({"nodes": N, "nnz": adj.channels[0].nnz, "steps": K, "targets": len(labels),
                  "fused_wall_s": round(t_fused, 4), "fused_stash_s": round(t_stash, 4), "fused_kernel_s": round(t_kernel, 4),
                  "fused_ms_per_target": round(1e3 * t_fused / len(labels), 4),
                  "composed_targets": len(sample), "composed_ms_per_target": round(1e3 * t_comp / len(sample), 3),
                  "node_ig_max_rel_diff_fused_vs_composed": agree, "device": torch.cuda.get_device_name(0)}))
