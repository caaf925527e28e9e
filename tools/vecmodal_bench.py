#!/usr/bin/env python3
"""Short-batch Dense + BatchNormalization + relu (csrc/shortm.hip) against the composed ops.dense -> ops.graph_bn route, which is
what sets ops.short_dense_fusion / ops.short_dense_max_rows.  One JSON line:

  layers   for the layers of the two model files (1437 -> 300, 300 -> 100, 100 -> 64, 114 -> 52, 37 -> 8; 1437 stands for the
           width of a real profeat table) at B = 50, 100, 256: forward + backward of the layer as it sits in a training step -- dX
           for every layer but a tower's first (1437 -> 300, 37 -> 8), the parameter gradients' second stages of the composed
           route deferred to one flush per four layers as a step does (ops.deferred_reductions) -- captured in a hipGraph of
           20 layer passes per replay; microseconds per layer pass, both routes
  steps    the whole captured training step (assembly, forward, loss, backward, Adam) of models.MultimodalVecGCN and
           models.MultimodalRegressionGCN on the stand-in dataset at the same batch sizes, microseconds per replay, both routes

Each figure is the median over --replays replays, each between two device synchronisations; the two routes alternate, and the
whole measurement runs twice (run 0, run 1): `spread` is the relative difference of the two runs' medians, the noise a
difference between the routes has to exceed.  `wins` lists the (rows, K, N) where the short route is ahead by more than that.
usage: python tools/vecmodal_bench.py [--replays 200] [--out profiles/vecmodal_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kgcn_amd import data_util as D, models, ops, train  # noqa: E402

dev = torch.device("cuda:0")
LAYERS = ((1437, 300, False), (300, 100, True), (100, 64, True), (114, 52, True), (37, 8, False))      # K, N, needs dX
BATCHES = (50, 100, 256)
COPIES, BODIES = 4, 5


def capture(body, warmup=3):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warmup):
            body()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        body()
    return g


def layer_graph(fused, B, K, N, dx):
    """a hipGraph of BODIES x COPIES forward + backward passes of the layer on the route `fused`"""
    ops.short_dense_fusion = fused
    gen = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=gen)
    xs = [rnd(B, K).requires_grad_(dx) for _ in range(COPIES)]
    dy = rnd(B, N)
    ps = [[(rnd(K, N) / K ** 0.5).requires_grad_(), rnd(N).requires_grad_(), (1 + 0.1 * rnd(N)).requires_grad_(),
           rnd(N).requires_grad_(), 0.1 * rnd(N), 0.5 + torch.rand(N, device=dev, generator=gen)] for _ in range(COPIES)]

    def body():
        for _ in range(BODIES):
            for t in xs + [p for q in ps for p in q[:4]]:
                t.grad = None
            ops.weight_tables.refresh()
            ys = [ops.dense_bn(x, *q, 1e-3, "relu") for x, q in zip(xs, ps)]
            with ops.deferred_reductions(root=ys):
                for y in ys:
                    y.backward(dy)

    g = capture(body)
    keep = (xs, ps, dy)
    return g, keep


def step_graph(fused, kind, B, reps=3):
    """the captured training step of a model on the stand-in dataset (tiled to 360 graphs) on the route `fused`"""
    ops.short_dense_fusion = fused
    z = np.load(os.path.join(ROOT, "tests", "golden", "g12_vecmodal.npz"))
    tile = lambda v: np.concatenate([v] * reps)
    regression = kind == "regression"
    channels, _ = D.build_adjs({"dense_adj": tile(z["ds_dense_adj"]), "max_node_num": int(z["ds_max_node_num"])})
    ds = D.DeviceGraphDataset(channels, tile(z["ds_feature"]), device=dev)
    sb = ds.static_batch(B)
    G = ds.num_graphs
    labels = sb.add_table(torch.as_tensor(tile(z["ds_label_reg"] if regression else z["ds_label_cls"]).astype(np.float32), device=dev))
    vec = tile(z["ds_dragon"]) if regression else np.tile(tile(z["ds_profeat"]), (1, 21))[:, :1437]      # a profeat-sized table
    kw = {"vectors": sb.add_table(torch.as_tensor(np.ascontiguousarray(vec, dtype=np.float32), device=dev))}
    if regression:
        mask = sb.add_table(torch.as_tensor(tile(z["ds_mask_label"]), device=dev))
        kw["enabled_node_nums"] = sb.add_table(torch.as_tensor(tile(z["ds_sizes"]).astype(np.int32), device=dev))
    else:
        mask = sb.add_table(torch.ones(G, device=dev))
    idx = np.random.default_rng(0).permutation(G)[:B]
    sb.load(idx)
    torch.manual_seed(0)
    model = (models.MultimodalRegressionGCN(2) if regression else models.MultimodalVecGCN(1, 2)).to(dev)
    with torch.no_grad():
        model(sb.features, sb.adjacency, **kw)
    opt = train.TFAdam(model.parameters(), lr=1e-3)
    step = train.GraphedTrainStep(model, opt, model.loss, sb, labels, mask, capture_assembly=True, **kw)
    return step.graph, (step, sb, model, opt)


def medians(graphs, replays, passes):
    """{name: [median of run 0, of run 1]} in microseconds per pass, the graphs alternating inside a run"""
    out = {name: [] for name in graphs}
    for _ in range(2):
        ts = {name: [] for name in graphs}
        for _ in range(replays):
            for name, g in graphs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                g.replay()
                torch.cuda.synchronize()
                ts[name].append((time.perf_counter() - t0) * 1e6 / passes)
        for name in graphs:
            out[name].append(float(np.median(ts[name])))
    return out


def compare(make, replays, passes):
    import gc
    gc.collect()                                                    # no dead hipGraph may be freed while a stream captures
    keep, graphs = [], {}
    for name, fused in (("short", True), ("composed", False)):
        g, k = make(fused)
        graphs[name] = g
        keep.append(k)
    for g in graphs.values():                                       # both warm before either is timed
        for _ in range(10):
            g.replay()
    m = medians(graphs, replays, passes)
    row = {}
    for name, (a, b) in m.items():
        row[name + "_us"] = (a + b) / 2
        row[name + "_runs_us"] = [a, b]
    row["spread"] = max(abs(a - b) / ((a + b) / 2) for a, b in m.values())
    row["short_over_composed"] = row["short_us"] / row["composed_us"]
    row["short_wins"] = bool(row["short_us"] < row["composed_us"] * (1.0 - row["spread"]))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    was = ops.short_dense_fusion
    layers, steps = [], []
    try:
        for B in BATCHES:
            for K, N, dx in LAYERS:
                row = dict(rows=B, k=K, n=N, dx=dx)
                row.update(compare(lambda fused: layer_graph(fused, B, K, N, dx), a.replays, COPIES * BODIES))
                layers.append(row)
                print("# layer", json.dumps(row), file=sys.stderr, flush=True)
        for kind in ("vec", "regression"):
            for B in BATCHES:
                row = dict(model=kind, rows=B)
                row.update(compare(lambda fused: step_graph(fused, kind, B), a.replays, 1))
                steps.append(row)
                print("# step", json.dumps(row), file=sys.stderr, flush=True)
    finally:
        ops.short_dense_fusion = was
    res = dict(layers=layers, steps=steps, replays=a.replays, passes_per_layer_replay=COPIES * BODIES,
               wins=[[r["rows"], r["k"], r["n"]] for r in layers if r["short_wins"]],
               max_spread=max(r["spread"] for r in layers + steps), device=torch.cuda.get_device_name(0))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
