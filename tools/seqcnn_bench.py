#!/usr/bin/env python3
"""Timings of the protein-sequence CNN (models.SeqCNN, sample_protein/sequence/cnn.py) at the sample's shape: L = 1,000 tokens,
26 symbols, embedding width 25, batch 1 (config_cnn.json) and 32.
  - per layer (the three conv-pool layers and the closing Conv1D(1, tanh)): HIP-event times of the forward kernel and of forward +
    backward (dX, dW, dbias, d table for the first layer; second stages inside the timed region), each beside the composed torch
    path with autograd -- F.embedding (first layer), F.conv1d on the SAME-padded input, relu / tanh, F.max_pool1d;
  - the whole captured training step (GraphedTrainStep replay).
Each figure is the median of --repeats measurements of --reps calls after a warm-up; the spread (max - min) / median is kept.
Prints one JSON line (and writes it to --out).

    python tools/seqcnn_bench.py [--length 1000] [--reps 20] [--repeats 5] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kgcn_amd import models, ops, train  # noqa: E402


def timed(fn, reps, repeats, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / reps)
    med = float(np.median(ms))
    return {"ms": round(med, 5), "spread": round((max(ms) - min(ms)) / med, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    L, S, E = args.length, 26, 25
    F = torch.nn.functional
    rng = np.random.default_rng(0)
    result = {"length": L, "symbols": S, "embedding_dim": E, "device": torch.cuda.get_device_name(0), "reps": args.reps,
              "repeats": args.repeats}
    for B in (1, 32):
        r = {}
        tok = torch.as_tensor(rng.integers(0, S, size=(B, L)).astype(np.int32), device=dev)
        torch.manual_seed(0)
        model = models.SeqCNN(S, embedding_dim=E).to(dev)
        model(None, None, sequences=tok)
        layers = list(model.convs) + [model.conv_out]
        x, Lin = None, L
        for i, lay in enumerate(layers, 1):
            k, p, Fo, act = lay.kernel_size, lay.pool, lay.filters, lay.activation
            w, b = lay.conv_kernel, lay.conv_bias
            cin = w.shape[1]
            g = torch.randn((B, Lin // p, Fo), device=dev)
            xin = None if i == 1 else x.detach().requires_grad_(True)
            kw = dict(tokens=tok, table=model.embeddings) if i == 1 else {}
            wrt = [model.embeddings if i == 1 else xin, w, b]
            with torch.no_grad():
                fwd = timed(lambda: ops.conv1d_pool(xin, w, b, p, act, **kw), args.reps, args.repeats)

            def both():
                torch.autograd.grad(ops.conv1d_pool(xin, w, b, p, act, **kw), wrt, g)

            fb = timed(both, args.reps, args.repeats)
            # composed torch yardstick (never on the product path)
            wt = w.detach().permute(2, 1, 0).contiguous().requires_grad_(True)                   # [F, Cin, k]
            bt = b.detach().clone().requires_grad_(True)
            emb = model.embeddings.detach().clone().requires_grad_(True)
            xt = None if i == 1 else x.detach().clone().requires_grad_(True)
            tok_long = tok.long()
            left = (k - 1) // 2

            def composed(grad=True):
                h = (F.embedding(tok_long, emb) if i == 1 else xt).transpose(1, 2)               # [B, Cin, L]
                y = F.conv1d(F.pad(h, (left, k - 1 - left)), wt, bt)
                y = torch.relu(y) if act == "relu" else torch.tanh(y)
                y = (F.max_pool1d(y, p) if p > 1 else y).transpose(1, 2)
                if grad:
                    torch.autograd.grad(y, [emb if i == 1 else xt, wt, bt], g)
                return y

            with torch.no_grad():
                cf = timed(lambda: composed(False), args.reps, args.repeats)
            cfb = timed(composed, args.reps, args.repeats)
            flops = 2.0 * B * (Lin // p * p) * k * cin * Fo
            r["layer%d" % i] = {"in": [B, Lin, cin], "filters": Fo, "kernel": k, "pool": p, "fwd": fwd, "fwd_bwd": fb,
                                "torch_fwd": cf, "torch_fwd_bwd": cfb, "fwd_gflops": round(flops / fwd["ms"] / 1e6, 1),
                                "fwd_speedup": round(cf["ms"] / fwd["ms"], 3), "fwd_bwd_speedup": round(cfb["ms"] / fb["ms"], 3)}
            with torch.no_grad():
                x = ops.conv1d_pool(xin, w, b, p, act, **kw)
            Lin //= p
        labels = torch.as_tensor(np.eye(2)[rng.integers(0, 2, size=B)], dtype=torch.float32, device=dev)
        mask = torch.ones(B, device=dev)
        opt = train.TFAdam(model.parameters(), lr=1e-4)

        class _SB:                                                                              # fixed buffers of the bench batch
            features, adjacency = None, None
        step = train.GraphedTrainStep(model, opt, model.loss, _SB, labels, mask, sequences=tok)
        r["train_step"] = timed(step.replay, args.reps, args.repeats)
        result["B%d" % B] = r
        del step, opt
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
