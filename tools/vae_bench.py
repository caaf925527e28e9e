#!/usr/bin/env python3
"""Graph VAE (example_model/model_vae.py) timings, one JSON line:
  step_ms        one captured training step (train.GraphedTrainStep replay: forward with its Philox noise, fused reconstruction
                 loss, backward, TF-Adam) at vae.json's shape (synthetic.jbl: 30 graphs, N = 10, F = 3, C = 1) and at a
                 ZINC-shaped synthetic batch (4,096 graphs, N = 70, F = 100, C = 1 and C = 6; sample_chem/generative_model)
  recon          the reconstruction term alone on the same data, forward + backward: the fused kernels (ops.vae_recon) against
                 the composed path (ops.gram per channel -> [B, C, N, N] logits -> torch sigmoid CE -> gram backward), with
                 each fused kernel's fraction of the HBM roof (8 TB/s, algorithmic bytes: Y read, dY written, CSR, features)
                 and of the fp32 matrix-pipe roof (157.3 TF; algorithmic flops of L = (Y w) Y^T and P = (G + G^T) Y).
usage: python tools/vae_bench.py [--steps K] [--warmup W] [--graphs B]"""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kgcn_amd import data_util as D, models, ops, train  # noqa: E402
from kgcn_amd.batched_csr import BatchedAdjacency  # noqa: E402

HBM_GBS = 8000.0
FP32_PIPE_TFLOPS = 157.3
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


def zinc_batch(B, N, C, F, seed=0):
    """Molecule-like graphs: a random spanning tree + 3 extra edges (symmetric), bond type per edge dealt to the C channels,
    self loops in channel 0; binary node features.  -> (BatchedAdjacency, features [B, N, F], dense labels [B, C, N, N])."""
    rng = np.random.default_rng(seed)
    child = np.tile(np.arange(1, N), B)
    g_tree = np.repeat(np.arange(B), N - 1)
    parent = (rng.random(B * (N - 1)) * child).astype(np.int64)
    g_x = np.repeat(np.arange(B), 3)
    xa, xb = rng.integers(0, N, B * 3), rng.integers(0, N, B * 3)
    keep = xa != xb
    g = np.concatenate([g_tree, g_x[keep]])
    r = np.concatenate([child, xa[keep]])
    c = np.concatenate([parent, xb[keep]])
    ch = rng.integers(0, C, g.shape[0])
    g, r, c, ch = np.concatenate([g, g]), np.concatenate([r, c]), np.concatenate([c, r]), np.concatenate([ch, ch])
    g = np.concatenate([g, np.repeat(np.arange(B), N)])
    r = np.concatenate([r, np.tile(np.arange(N), B)])
    c = np.concatenate([c, np.tile(np.arange(N), B)])
    ch = np.concatenate([ch, np.zeros(B * N, np.int64)])
    order = np.lexsort((c, r, g))
    g, r, c, ch = g[order], r[order], c[order], ch[order]
    chans = []
    dense = torch.zeros((B, C, N, N), device=dev)
    for k in range(C):
        s = ch == k
        t = [torch.from_numpy(a[s].astype(np.int32)).to(dev) for a in (g, r, c)]
        chans.append((t[0], t[1], t[2], torch.ones(int(s.sum()), device=dev)))
        dense[t[0].long(), k, t[1].long(), t[2].long()] = 1.0
    adj = BatchedAdjacency.from_device_coo(chans, B, N)
    x = torch.from_numpy((rng.random((B, N, F)) < 0.1).astype(np.float32)).to(dev)
    return adj, x, dense


def step_ms(model, features, adj, mask, steps, warmup):
    model(features, adj, graph_mask=mask)
    opt = train.TFAdam(model.parameters(), lr=1e-4)
    model.bind_step(opt._t_dev)
    sb = types.SimpleNamespace(features=features, adjacency=adj)
    step = train.GraphedTrainStep(model, opt, model.loss, sb, mask, mask, graph_mask=mask)
    return timed(step.replay, steps, warmup)


def recon_compare(adj, x, dense, C, steps, warmup, seed=0):
    B, N, F = x.shape
    g = torch.Generator(device=dev).manual_seed(seed)
    ys = [torch.rand((B, N, 64), device=dev, generator=g).requires_grad_(True) for _ in range(C)]
    ws = [((torch.rand(64, device=dev, generator=g) - 0.5) * 0.4).requires_grad_(True) for _ in range(C)]
    xf = torch.randn((B, N, F), device=dev, generator=g).requires_grad_(True)
    mask = torch.ones(B, device=dev)
    params = ys + ws + [xf]

    def fused_fwd():
        return ops.vae_recon(adj, ys, ws, xf, x, mask)

    def fused():
        co, _, _ = fused_fwd()
        torch.autograd.grad(co, params)

    def composed():
        logits = torch.stack([ops.gram(y, w) for y, w in zip(ys, ws)], dim=1)
        link = torch.nn.functional.binary_cross_entropy_with_logits(logits, dense, reduction="none").mean(dim=(1, 2, 3))
        feat = torch.nn.functional.binary_cross_entropy_with_logits(xf, x, reduction="none").mean(dim=(1, 2))
        co = (mask * (feat + link)).mean()
        torch.autograd.grad(co, params)

    fwd_ms = timed(lambda: fused_fwd(), steps, warmup)
    both_ms = timed(fused, steps, warmup)
    comp_ms = timed(composed, steps, warmup)
    # agreement of the two paths on these data (cost and dY of channel 0)
    co_f = fused_fwd()[0]
    gf = torch.autograd.grad(co_f, ys[0])[0]
    logits = torch.stack([ops.gram(y, w) for y, w in zip(ys, ws)], dim=1)
    link = torch.nn.functional.binary_cross_entropy_with_logits(logits, dense, reduction="none").mean(dim=(1, 2, 3))
    feat = torch.nn.functional.binary_cross_entropy_with_logits(xf, x, reduction="none").mean(dim=(1, 2))
    co_c = (mask * (feat + link)).mean()
    gc = torch.autograd.grad(co_c, ys[0])[0]
    agree = dict(cost_rel=abs(float(co_f) - float(co_c)) / abs(float(co_c)),
                 dy_rel=float((gf - gc).abs().max() / gc.abs().max()))
    nnz = sum(int(ch.nnz) for ch in adj.channels)
    csr = sum(4 * (B * N + 1) + 8 * int(ch.nnz) for ch in adj.channels)
    y_bytes = 4 * B * N * 64 * C
    f_bytes = 4 * B * N * F
    fwd_bytes = y_bytes + csr + 2 * f_bytes
    bwd_bytes = 2 * y_bytes + csr + 3 * f_bytes
    fwd_flops = 2.0 * B * C * N * N * 64
    bwd_flops = 2 * fwd_flops
    bwd_ms = both_ms - fwd_ms
    return dict(fused_fwd_us=1e3 * fwd_ms, fused_bwd_us=1e3 * bwd_ms, fused_fwd_bwd_us=1e3 * both_ms,
                composed_fwd_bwd_us=1e3 * comp_ms, speedup=comp_ms / both_ms, nnz=nnz,
                fwd_frac_hbm=fwd_bytes / (fwd_ms * 1e-3) / (HBM_GBS * 1e9),
                bwd_frac_hbm=bwd_bytes / (bwd_ms * 1e-3) / (HBM_GBS * 1e9),
                fwd_frac_fp32_pipe=fwd_flops / (fwd_ms * 1e-3) / (FP32_PIPE_TFLOPS * 1e12),
                bwd_frac_fp32_pipe=bwd_flops / (bwd_ms * 1e-3) / (FP32_PIPE_TFLOPS * 1e12), agreement=agree)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--graphs", type=int, default=4096)
    args = ap.parse_args()
    out = dict(metric="vae", device=torch.cuda.get_device_name(0))
    # vae.json: synthetic.jbl, batch 30
    raw = np.load(os.path.join(ROOT, "tests", "golden", "g1_synthetic_raw.npz"))
    channels, _ = D.build_adjs({"dense_adj": raw["dense_adj"].astype(np.int64), "max_node_num": int(raw["max_node_num"])})
    ds = D.DeviceGraphDataset(channels, raw["feature"], device=dev)
    adj, x = ds.batch(np.arange(30), 30)
    torch.manual_seed(0)
    out["step_ms_vae_json"] = step_ms(models.GraphVAE(x.shape[2], 1).to(dev), x, adj, torch.ones(30, device=dev),
                                      args.steps, args.warmup)
    B, N, F = args.graphs, 70, 100
    for C in (1, 6):
        adj, x, dense = zinc_batch(B, N, C, F, seed=C)
        torch.manual_seed(0)
        out["step_ms_zinc_c%d" % C] = step_ms(models.GraphVAE(F, C).to(dev), x, adj, torch.ones(B, device=dev),
                                              args.steps, args.warmup)
        out["recon_zinc_c%d" % C] = recon_compare(adj, x, dense, C, args.steps, args.warmup)
        del adj, x, dense
        torch.cuda.empty_cache()
    out["shape_zinc"] = dict(graphs=B, nodes=N, features=F, latent=64)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
