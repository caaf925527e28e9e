#!/usr/bin/env python3
"""Timings of the multimodal model (models.MultimodalGCN, example_model/model_multimodal.py) at a compound-protein-shaped
synthetic batch: 4,096 pairs, <= 50 atoms, 81 atom features, L = 700 tokens, S = 25 symbols, E = 4 and 25.
  - per-kernel HIP-event times of the sequence branch (conv-pool and LSTM, forward and backward, the deferred second stages
    flushed inside the timed region), and the whole captured training step (GraphedTrainStep replay);
  - the fused sequence branch (forward + backward) against a composed torch version -- F.embedding + F.conv1d (SAME: 1 left,
    2 right) + relu + F.max_pool1d + nn.LSTM (sigmoid gates, time-reversed input) -- a timing yardstick only.
Prints one JSON line (and writes it to --out).

    python tools/multimodal_bench.py [--pairs 4096] [--reps 20] [--out FILE]
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
from kgcn_amd.batched_csr import as_batched_adjacency  # noqa: E402
from oracle import kgcn_oracle as K  # noqa: E402


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, N, Fa, L, S = args.pairs, 50, 81, 700, 25
    rng = np.random.default_rng(0)
    adjs = K.synth_mol_graphs(rng, B, N, 3)
    adj = as_batched_adjacency(adjs, n_nodes=N, device=dev)
    feats = torch.as_tensor(rng.standard_normal((B, N, Fa)).astype(np.float32) * 0.3, device=dev)
    tok = rng.integers(1, S, size=(B, L)).astype(np.int32)
    tok[np.arange(L)[None, :] >= rng.integers(L // 4, L + 1, size=B)[:, None]] = 0
    tok = torch.as_tensor(tok, device=dev)
    labels = torch.as_tensor(np.eye(2)[rng.integers(0, 2, size=B)], dtype=torch.float32, device=dev)
    mask = torch.ones(B, device=dev)
    result = {"pairs": B, "atoms": N, "atom_features": Fa, "length": L, "symbols": S, "device": torch.cuda.get_device_name(0)}
    for E in (4, 25):
        r = {}
        torch.manual_seed(0)
        model = models.MultimodalGCN(S, embedding_dim=E).to(dev)
        model(feats, adj, sequences=tok)
        enc = model.sequence
        T = L // 4
        g_pool = torch.randn((B, T, 50), device=dev)
        g_h = torch.randn((B, 32), device=dev)
        with torch.no_grad():
            r["convpool_fwd_ms"] = timed(lambda: ops.seq_conv_pool(tok, enc.embeddings, enc.conv_kernel, enc.conv_bias, 4), args.reps)
            pooled = ops.seq_conv_pool(tok, enc.embeddings, enc.conv_kernel, enc.conv_bias, 4)
            r["lstm_fwd_ms"] = timed(lambda: ops.seq_lstm(pooled, enc.kernel, enc.recurrent_kernel, enc.bias), args.reps)

        def cp_bwd():
            out = ops.seq_conv_pool(tok, enc.embeddings, enc.conv_kernel, enc.conv_bias, 4)
            torch.autograd.grad(out, [enc.embeddings, enc.conv_kernel, enc.conv_bias], g_pool)

        def lstm_bwd():
            x = pooled.detach().requires_grad_(True)
            h = ops.seq_lstm(x, enc.kernel, enc.recurrent_kernel, enc.bias)
            torch.autograd.grad(h, [x, enc.kernel, enc.recurrent_kernel, enc.bias], g_h)

        def fused_branch():
            h = enc(tok)
            torch.autograd.grad(h, list(enc.parameters()), g_h)

        r["convpool_fwd_train_plus_bwd_ms"] = timed(cp_bwd, args.reps)
        r["convpool_bwd_ms"] = r["convpool_fwd_train_plus_bwd_ms"] - r["convpool_fwd_ms"]
        r["lstm_fwd_train_plus_bwd_ms"] = timed(lstm_bwd, args.reps)
        r["lstm_bwd_ms"] = r["lstm_fwd_train_plus_bwd_ms"] - r["lstm_fwd_ms"]
        r["fused_sequence_branch_fwd_bwd_ms"] = timed(fused_branch, args.reps)

        # composed torch yardstick (never on the product path)
        emb = enc.embeddings.detach().clone().requires_grad_(True)
        wconv = enc.conv_kernel.detach().permute(2, 1, 0).contiguous().requires_grad_(True)     # [F, E, k]
        bconv = enc.conv_bias.detach().clone().requires_grad_(True)
        lstm = torch.nn.LSTM(50, 32, batch_first=True).to(dev)
        tok_long = tok.long()

        def composed_branch():
            x = torch.nn.functional.embedding(tok_long, emb).transpose(1, 2)                   # [B, E, L]
            y = torch.relu(torch.nn.functional.conv1d(torch.nn.functional.pad(x, (1, 2)), wconv, bconv))
            p = torch.nn.functional.max_pool1d(y, 4).transpose(1, 2)                            # [B, T', F]
            _, (hn, _) = lstm(p.flip(1))
            torch.autograd.grad(hn[0], [emb, wconv, bconv] + list(lstm.parameters()), g_h)

        r["composed_torch_branch_fwd_bwd_ms"] = timed(composed_branch, args.reps)
        r["fused_speedup"] = r["composed_torch_branch_fwd_bwd_ms"] / r["fused_sequence_branch_fwd_bwd_ms"]

        opt = train.TFAdam(model.parameters(), lr=1e-3)

        class _SB:                                                                         # fixed buffers of the bench batch
            features, adjacency = feats, adj
        step = train.GraphedTrainStep(model, opt, models.MultimodalGCN.loss, _SB, labels, mask, sequences=tok)
        r["train_step_ms"] = timed(step.replay, args.reps)
        r["stash_bytes"] = int(ops.lib.kgcn_seq_lstm_stash_floats(B, T, 32)) * 4
        r["pooled_bytes"] = B * T * 50 * 4
        result["E%d" % E] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}
        del step, opt
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
