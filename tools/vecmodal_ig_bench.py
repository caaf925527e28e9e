#!/usr/bin/env python3
"""Integrated gradients over the vector modality at the reference's size: C = 256 compounds of N = 50 nodes and F = 81 features,
D = 100 steps (101 copies), the vector Dv = 1437 wide for models.MultimodalVecGCN (profeat, first layer 1437 -> 300) and Dv = 37
for models.MultimodalRegressionGCN (dragon, first layer 37 -> 8).

  fused     visualization.vecmodal_integrated_gradients(fused=True): v W once per compound, ops.ig_copies_expand over the copies,
            ops.ig_copies_reduce and one [C, H] x W^T product (csrc/vecig.hip).
  composed  fused=False: the scaled vectors as batch rows through the model's own first layer, autograd to them -- the path the
            ops of this package gave before the two kernels, the only comparator.
  loop      one batch-1 forward + backward per step and compound through the same chunk function (forward only for the start
            copy), on --loop-compounds compounds: the reference's loop.
  kernels   the two entry points alone at [C (D + 1), H] (50 launches per timed window), against their algorithmic bytes: C K H floats written by expand (P, bias and
            the normalisation's vectors are C H + 5 H floats read), 2 C K H floats read by reduce (C H written).

Whole calls (modal = the vector alone, and 'all') and kernels are timed with device events over --repeats runs after a warm-up of
the same shapes, the two routes alternating; reported are the median and the smallest and largest run.  Prints one JSON line;
--out writes it to a file as well.  No threshold: `fused_default` records which route is ahead per model, which is what
visualization.VECMODAL_IG_FUSED holds.

    python tools/vecmodal_ig_bench.py [--repeats 20] [--loop-compounds 2] [--out profiles/vecmodal_ig_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kgcn_amd import _lib, data_util as D, models, ops, visualization as V  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--loop-compounds", type=int, default=2)
ap.add_argument("--compounds", type=int, default=256)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda:0")
N, F, G, STEPS = 50, 81, args.compounds, args.steps
rng = np.random.default_rng(0)
dense = np.zeros((G, N, N), np.float32)
x = np.zeros((G, N, F), np.float32)
sizes = np.zeros(G, np.int32)
for g in range(G):                                           # molecule-like graphs: self loops and about three bonds a node
    m = sizes[g] = int(rng.integers(20, N + 1))
    x[g, :m] = rng.standard_normal((m, F))
    for i in range(m):
        dense[g, i, i] = 1.0
        for j in rng.integers(0, m, size=3):
            dense[g, i, j] = dense[g, j, i] = 1.0
dataset = D.DeviceGraphDataset([D.FlatAdjacency.from_dense(dense)], x, device=dev)


def timed(fns, repeats):
    """The callables of `fns` alternating, each `repeats` times after one warm-up -> per callable the milliseconds of every run."""
    for fn in fns:
        fn()
    ms = [[] for _ in fns]
    for _ in range(repeats):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b))
    return ms


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4), "max_ms": round(float(np.max(ms)), 4)}


def loop_route(model, vtab, sz, cids, modal):
    """The reference's loop: one batch-1 pass per step and compound, the weighted gradients summed on the host side of the loop."""
    targets, name = V.vecmodal_ig_targets(model, modal)
    plan = V.ig_row_plan("ig", STEPS)
    first = V._vecmodal_first_layer(model)
    mask = np.array([[1.0, 0.0]], np.float32)
    out = []
    for cid in cids:
        total = None
        for k, w in enumerate(plan.weights):
            r = V._vecmodal_chunk(model, dataset, vtab, sz, [cid], V.ig_plan_row(plan, k), targets, name, mask, first, False,
                                  need_grad=w != 0.0)
            total = r[name] if total is None else total + r[name]
        out.append(total)
    return out


result = {"compounds": G, "nodes": N, "features": F, "steps": STEPS, "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
          "timing": "device events around each call, the routes alternating; median, smallest and largest of `repeats` runs"}
for kind, Dv in (("vec", 1437), ("regression", 37)):
    torch.manual_seed(0)
    model = (models.MultimodalRegressionGCN(2) if kind == "regression" else models.MultimodalVecGCN(1, 2)).to(dev)
    vtab = torch.as_tensor(rng.standard_normal((G, Dv)).astype(np.float32) * 0.3, device=dev)
    sz = torch.as_tensor(sizes, device=dev) if kind == "regression" else None
    with torch.no_grad():
        adj, xb = dataset.batch(np.arange(4))
        model(xb, adj, vectors=vtab[:4])
    for p in model.parameters():
        p.requires_grad_(False)
    name = V.VECMODAL_VECTOR_NAMES[type(model).__name__]
    H = (model.vec if kind == "regression" else model.tower[0]).units
    entry = {"vector_width": Dv, "first_layer_width": H}
    for modal in (name, "all"):
        call = lambda fused, modal=modal: V.vecmodal_integrated_gradients(model, None, dataset, vtab, divide_number=STEPS, modal=modal,
                                                                          fused=fused, enabled_node_nums=sz)
        ms_f, ms_c = timed([lambda: call(True), lambda: call(False)], args.repeats)
        a, b = call(True), call(False)
        big = max(float(np.abs(r[name + "_IG"]).max()) for r in a)
        diff = max(float(np.abs(p[name + "_IG"] - q[name + "_IG"]).max()) for p, q in zip(a, b)) / big
        entry["modal_" + modal] = {"fused": stats(ms_f), "composed": stats(ms_c),
                                   "composed_over_fused": round(float(np.median(ms_c) / np.median(ms_f)), 3),
                                   "vector_IG_max_rel_diff_fused_vs_composed": diff}
    nl = max(1, min(args.loop_compounds, G))
    (ms_l,) = timed([lambda: loop_route(model, vtab, sz, range(nl), name)], max(1, min(args.repeats, 3)))
    entry["loop"] = dict(stats(ms_l), compounds=nl, ms_per_compound=round(float(np.median(ms_l)) / nl, 3),
                         fused_ms_per_compound=round(entry["modal_" + name]["fused"]["median_ms"] / G, 4),
                         composed_ms_per_compound=round(entry["modal_" + name]["composed"]["median_ms"] / G, 4))
    # the two kernels alone: the entry points themselves, INNER launches per timed window
    K, INNER = STEPS + 1, 50
    layer = model.vec if kind == "regression" else model.tower[0]
    scales, weights = V.ig_scales("ig", STEPS)
    P, Y, S = torch.randn((G, H), device=dev), torch.empty((G * K, H), device=dev), torch.empty((G, H), device=dev)
    dY, sc = torch.randn((G * K, H), device=dev), torch.ones(H, device=dev)
    al, wt = torch.tensor(scales, device=dev, dtype=torch.float32), torch.tensor(weights, device=dev, dtype=torch.float32)
    ptr, stream, relu = _lib.ptr, _lib.current_stream(), ops.act_code("relu")

    def expand():
        for _ in range(INNER):
            _lib.check(_lib.lib.kgcn_ig_copies_expand_f32(ptr(P), G, K, H, ptr(al), ptr(layer.bias), ptr(layer.gamma), ptr(layer.beta),
                                                          ptr(layer.moving_mean), ptr(layer.moving_variance), layer.eps, relu, ptr(Y), H,
                                                          stream), "expand")

    def reduce():
        for _ in range(INNER):
            _lib.check(_lib.lib.kgcn_ig_copies_reduce_f32(ptr(dY), H, ptr(Y), H, G, K, H, ptr(wt), ptr(sc), relu, ptr(S), stream), "reduce")

    ms_e, ms_r = ([t / INNER for t in ms] for ms in timed([expand, reduce], args.repeats))
    eb, rb = 4 * (G * K * H + G * H + 5 * H), 4 * (2 * G * K * H + G * H)
    entry["kernels"] = {"rows": G * K, "launches_per_window": INNER,
                        "expand": dict(stats(ms_e), bytes=eb, gb_per_s=round(eb / np.median(ms_e) / 1e6, 1)),
                        "reduce": dict(stats(ms_r), bytes=rb, gb_per_s=round(rb / np.median(ms_r) / 1e6, 1))}
    entry["fused_default"] = bool(entry["modal_" + name]["composed_over_fused"] > 1.0 and entry["modal_all"]["composed_over_fused"] > 1.0)
    result[kind] = entry
line = json.dumps(result)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
