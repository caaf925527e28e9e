#!/usr/bin/env python3
"""Timings of integrated gradients for the multimodal model (visualization.multimodal_integrated_gradients) at the
compound-protein shape: N = 50 atoms, 81 atom features, L = 700 tokens, S = E = 25, D = 100 steps, modal 'all', method 'ig'.
  - the batched attribution (the D + 1 scaled copies of every compound as rows of one forward + one backward) per compound, at
    C = 1, 16 and 256 compounds;
  - the per-step loop through the same ops (batched=False: D + 1 batch-1 passes per compound, rep = 1) per compound;
  - the conv-pool input-gradient kernel alone (ops.seq_conv_pool_input_grad, HIP events) on the rows of one chunk.
Prints one JSON line (and writes it to --out).

    python tools/multimodal_ig_bench.py [--loop-compounds 2] [--out FILE]
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
from oracle import kgcn_oracle as K  # noqa: E402


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loop-compounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    Cmax, N, Fa, L, S, E, Dn = 256, 50, 81, 700, 25, 25, 100
    rng = np.random.default_rng(0)
    adjs = K.synth_mol_graphs(rng, Cmax, N, 3)
    channels = [D.FlatAdjacency.from_coo_list([a[0] for a in adjs], N)]
    x = (rng.standard_normal((Cmax, N, Fa)) * 0.3).astype(np.float32)
    tok = torch.as_tensor(rng.integers(0, S, size=(Cmax, L)).astype(np.int32), device=dev)
    dataset = D.DeviceGraphDataset(channels, x, device=dev)
    torch.manual_seed(0)
    model = models.MultimodalGCN(S, embedding_dim=E, label_dim=2).to(dev)
    adj, xx = dataset.batch(np.arange(4))
    model(xx, adj, sequences=tok[:4])
    result = {"atoms": N, "atom_features": Fa, "length": L, "symbols": S, "embed_dim": E, "divide_number": Dn, "modal": "all",
              "method": "ig", "rows_per_chunk": V.IG_ROWS_PER_CHUNK // (Dn + 1) * (Dn + 1),
              "device": torch.cuda.get_device_name(0)}
    V.multimodal_integrated_gradients(model, None, dataset, tok, divide_number=Dn, compounds=[0])       # warm-up
    batched = {}
    for C in (1, 16, 256):
        t, res = wall(lambda: V.multimodal_integrated_gradients(model, None, dataset, tok, divide_number=Dn,
                                                                compounds=list(range(C))))
        batched[str(C)] = {"seconds": round(t, 4), "ms_per_compound": round(1e3 * t / C, 3),
                           "max_abs_sum_of_IG_minus_check_score": float(max(abs(r["sum_of_IG"] - r["check_score"]) for r in res))}
        print("batched C = %d: %.1f ms per compound" % (C, 1e3 * t / C), flush=True)
    result["batched"] = batched
    nl = args.loop_compounds
    V.multimodal_integrated_gradients(model, None, dataset, tok, divide_number=2, compounds=[0], batched=False)   # warm-up
    t, _ = wall(lambda: V.multimodal_integrated_gradients(model, None, dataset, tok, divide_number=Dn, compounds=list(range(nl)),
                                                          batched=False))
    result["loop"] = {"compounds": nl, "seconds": round(t, 4), "ms_per_compound": round(1e3 * t / nl, 3)}
    print("loop: %.1f ms per compound" % (1e3 * t / nl), flush=True)
    for C in ("1", "16", "256"):
        batched[C]["speedup_over_loop"] = round(result["loop"]["ms_per_compound"] / batched[C]["ms_per_compound"], 2)
    # the input-gradient kernel alone, on the rows of one chunk of each C
    seqm = model.sequence
    kern = {}
    for C in (1, 16, min(256, V.IG_ROWS_PER_CHUNK // (Dn + 1))):
        R = C * (Dn + 1)
        scale = torch.arange(Dn + 1, device=dev, dtype=torch.float32).repeat(C) / Dn
        pooled, arg = ops.seq_conv_pool_scaled(tok[:C], seqm.embeddings.detach(), seqm.conv_kernel.detach(), seqm.conv_bias.detach(),
                                               4, scale, Dn + 1, argmax=True)
        g = torch.randn_like(pooled)
        wt = torch.full((R,), 1.0 / Dn, device=dev)
        wt[::Dn + 1] = 0
        run = lambda: ops.seq_conv_pool_input_grad(g, arg, tok[:C], seqm.embeddings.detach(), seqm.conv_kernel.detach(), 4, Dn + 1,
                                                   row_weight=wt, times_table=True)
        for _ in range(3):
            run()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(10):
            run()
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b) / 10
        kern[str(C)] = {"rows": R, "ms": round(ms, 4), "us_per_compound": round(1e3 * ms / C, 2)}
        print("input-gradient kernel, %d compounds (%d rows): %.3f ms" % (C, R, ms), flush=True)
    result["input_grad_kernel"] = kern
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
