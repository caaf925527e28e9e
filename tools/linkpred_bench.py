#!/usr/bin/env python3
"""Knowledge-graph link prediction (sample_kg/network_prediction) timings, one JSON line:
  step_ms     one captured training step per model (train.GraphedTrainStep replay: label batch assembly with the Philox negatives,
              model, ranking loss, backward, TF-Adam) on the BA fixture (N = 5,000, D = 128, L = 1,000)
  loss        the ranking loss alone, forward + backward, for gcn and distmult: the fused kernels (ops.linkpred_loss) against
              the composed torch form (index_select of the four rows, products, sums, cost, autograd backward = index_add_) at
              the sample shape and at a synthetic Barabasi-Albert shape (N = 100,000, m = 10, L = 65,536)
  sum_pass    the store-and-sum kernels of the backward (chunk pass + per-node pass) from a torch.profiler trace: time and
              algorithmic bytes (per entry its 8-B index pair, 24-B label row, partner row and, for distmult, relation row; every
              dH row written once) with the fraction of the HBM roof (8 TB/s)
usage: python tools/linkpred_bench.py [--steps K] [--warmup W] [--out profiles/linkpred_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kgcn_amd import data_util as D, models, ops, train  # noqa: E402

HBM_GBS = 8000.0
dev = torch.device("cuda:0")


def timed(fn, steps, warmup):
    """median ms of fn() over `steps` runs (CUDA events around each, after `warmup` runs)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def fixture():
    z = np.load(os.path.join(ROOT, "tests", "golden", "g8_kg_linkpred.npz"))
    return D.LinkPredictionData({"adj": [(z["adj_idx"], z["adj_val"], np.array([int(z["node_num"])] * 2))], "node": z["node"],
                                 "node_num": z["node_num"], "label_list": z["label_list"],
                                 "test_label_list": z["test_label_list"]})


def step_ms(variant, data, steps, warmup):
    tr, _ = D.split_label_list(data.label_list, 0.2, np.random.RandomState(0))
    adj = data.adjacency(dev) if variant == "gcn" else None
    feed = D.LinkPredFeed(tr, batch=1000, adjacency=adj, device=dev)
    torch.manual_seed(0)
    model = models.LinkPredictionNet(variant, data.num_nodes, data.num_relations, seed=1, device=dev)
    model(None, adj, feed=feed)
    opt = train.TFAdam(model.parameters(), lr=1e-3)
    model.bind_step(opt._t_dev)
    g = train.GraphedTrainStep(model, opt, model.loss, feed, None, None, feed=feed)
    return timed(g.replay, steps, warmup)


def ba_labels(N, m, L, rng):
    """Label rows of a Barabasi-Albert graph (preferential attachment, m edges per new node): L positive edges drawn from it."""
    rep = np.empty(2 * m * N, np.int64)            # every edge end so far: a uniform pick is a pick by degree
    rep[:m], n = np.arange(m), m
    src, dst = [], []
    for v in range(m, N):
        t = np.unique(rep[rng.integers(0, n, m)]) if v > m else np.arange(m)
        src.append(np.full(len(t), v))
        dst.append(t)
        rep[n:n + len(t)] = t
        rep[n + len(t):n + 2 * len(t)] = v
        n += 2 * len(t)
    src, dst = np.concatenate(src), np.concatenate(dst)
    e = rng.integers(0, len(src), L)
    lab = np.zeros((L, 6), np.int64)
    lab[:, 0], lab[:, 1], lab[:, 2] = src[e], 2, dst[e]
    lab[:, 3], lab[:, 5] = lab[:, 0], rng.integers(0, N, L)
    return lab


def composed(h, w, rows, mode):
    r = rows.long()
    p0, p1, p2, p3 = (h.index_select(0, r[:, c]) for c in (0, 2, 3, 5))
    if mode == "distmult":
        s1 = (p0 * p1 * w.index_select(0, r[:, 1])).sum(1)
        s2 = (p2 * p3 * w.index_select(0, r[:, 4])).sum(1)
        cost = -torch.log(1.0 / (1.0 + torch.exp(s2 - s1 + 0.1)) + 1e-10)
    else:
        s1, s2 = (p0 * p1).sum(1), (p2 * p3).sum(1)
        cost = -torch.log(torch.sigmoid(s1 - s2) + 1e-10)
    return cost.mean()


def loss_case(mode, N, lab, steps, warmup):
    rng = np.random.default_rng(1)
    L = len(lab)
    feed = D.LinkPredFeed(lab, batch=L, device=dev)
    h = torch.as_tensor(rng.standard_normal((N, 128)).astype(np.float32) * 0.1, device=dev).requires_grad_(True)
    w = torch.as_tensor(rng.standard_normal((3, 128)).astype(np.float32), device=dev).requires_grad_(True) \
        if mode == "distmult" else None
    step = torch.zeros((), dtype=torch.int64, device=dev)

    def fused():
        c, *_ = ops.linkpred_loss(h, feed, mode, w=w, seed=3, step=step)
        c.backward()

    _, _, _, _, _, rows = ops.linkpred_loss(h, feed, mode, w=w, seed=3, step=step)
    rows = rows.detach()

    def comp():
        composed(h, w, rows, mode).backward()

    out = dict(mode=mode, N=N, L=L, fused_ms=timed(fused, steps, warmup), composed_ms=timed(comp, steps, warmup))
    cnt = np.bincount(np.concatenate([lab[:, 0], lab[:, 2], lab[:, 0], rows[:, 5].cpu().numpy()]), minlength=N)
    out.update(entries_per_node_max=int(cnt.max()), entries_per_node_median_nonzero=float(np.median(cnt[cnt > 0])))
    # the sum pass from a profiler trace
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(5):
                fused()
            torch.cuda.synchronize()
        us = {}
        for ev in prof.key_averages():
            for name in ("lp_chunk_sum_kernel", "lp_node_sum_kernel"):
                if name in ev.key:
                    us[name] = us.get(name, 0.0) + ev.device_time_total / 5.0
        E = 4 * L
        # gathered: what the kernels load and store as written; compulsory: every byte once (H and dH once, the index once)
        gathered = E * (8 + 24 + 4 + 128 * 4 * (2 if mode == "distmult" else 1)) + N * 128 * 4 + 2 * (N + 1) * 4
        compulsory = E * 8 + L * 28 + 2 * N * 128 * 4 + (N + 1) * 4
        t = sum(us.values()) * 1e-6
        out["sum_pass"] = dict(kernels_us={k: round(v, 2) for k, v in us.items()}, gathered_bytes=int(gathered),
                               compulsory_bytes=int(compulsory),
                               frac_hbm_compulsory=(compulsory / t / (HBM_GBS * 1e9)) if t > 0 else None)
    except Exception as e:                                            # noqa: BLE001  (a trace is evidence, not a requirement)
        out["sum_pass"] = dict(error=str(e)[:200])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    data = fixture()
    res = dict(step_ms={v: step_ms(v, data, a.steps, a.warmup) for v in ("gcn", "distmult", "ip")}, loss=[])
    rng = np.random.default_rng(0)
    tr = data.label_list[:1000].astype(np.int64)
    big = ba_labels(100000, 10, 65536, rng)
    for mode in ("gcn", "distmult"):
        res["loss"].append(loss_case(mode, data.num_nodes, tr, a.steps, a.warmup))
        res["loss"].append(loss_case(mode, 100000, big, a.steps, a.warmup))
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
