#!/usr/bin/env python3
"""Timings of integrated gradients for the multimodal model (visualization.multimodal_integrated_gradients) at the
compound-protein shape: N = 50 atoms, 81 atom features, L = 700 tokens, S = E = 25, D = 100 steps, modal 'all', method 'ig'.
  - the batched attribution (the D + 1 scaled copies of every compound as rows of one forward + one backward) per compound, at
    C = 1, 16 and 256 compounds;
  - the per-step loop through the same ops (batched=False: D + 1 batch-1 passes per compound, rep = 1) per compound;
  - the conv-pool input-gradient kernel alone (ops.seq_conv_pool_input_grad, HIP events) on the rows of one chunk;
  - the smooth methods (noise drawn on the device): the noisy conv-pool forward (ops.seq_conv_pool_perturbed, D + 2 copies a
    compound, D of them noisy) beside the clean scaled forward on the same rows, alternating in one process (HIP events); the
    whole 'smooth_ig' attribution beside 'ig' on the same compounds, alternating; and its batched form beside batched=False.
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
    # ---- the smooth methods: noise drawn on the device ----
    rep = Dn + 2
    scales, sigmas, samples, _, _, _ = V.smooth_rows("smooth_ig", Dn, 0.1)
    conv = {}
    for C in (1, 16, V.IG_ROWS_PER_CHUNK // rep):
        sc = torch.tensor(scales, device=dev, dtype=torch.float32).repeat(C)
        sg = torch.tensor(sigmas, device=dev, dtype=torch.float32).repeat(C)
        smp = torch.tensor(samples, device=dev, dtype=torch.int32).repeat(C)
        ids = torch.arange(C, device=dev, dtype=torch.int32)
        cargs = (tok[:C], seqm.embeddings.detach(), seqm.conv_kernel.detach(), seqm.conv_bias.detach(), 4, sc, rep)
        arms = {"clean_scaled": lambda: ops.seq_conv_pool_scaled(*cargs, argmax=True),
                "perturbed": lambda: ops.seq_conv_pool_perturbed(*cargs, sg, smp, ids, 1234, argmax=True)}
        for fn in arms.values():
            for _ in range(3):
                fn()
        ms = {k: [] for k in arms}
        for _ in range(7):                                           # alternate the two arms
            for name, fn in arms.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(5):
                    fn()
                b.record()
                b.synchronize()
                ms[name].append(a.elapsed_time(b) / 5)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        conv[str(C)] = {"rows": C * rep, "noisy_rows": C * Dn, "clean_scaled_ms": round(med["clean_scaled"], 4),
                        "perturbed_ms": round(med["perturbed"], 4), "ratio": round(med["perturbed"] / med["clean_scaled"], 3),
                        "clean_scaled_ms_min_max": [round(min(ms["clean_scaled"]), 4), round(max(ms["clean_scaled"]), 4)],
                        "perturbed_ms_min_max": [round(min(ms["perturbed"]), 4), round(max(ms["perturbed"]), 4)]}
        print("conv-pool forward, %d rows: clean %.3f ms, perturbed %.3f ms (x%.2f)"
              % (C * rep, med["clean_scaled"], med["perturbed"], med["perturbed"] / med["clean_scaled"]), flush=True)
    result["smooth_conv_pool_forward"] = conv
    V.multimodal_integrated_gradients(model, None, dataset, tok, divide_number=Dn, compounds=[0], method="smooth_ig")   # warm-up
    whole = {}
    for C in (1, 16, 256):
        t = {"ig": [], "smooth_ig": []}
        for _ in range(3):                                               # alternate the two methods
            for m in t:
                t[m].append(wall(lambda: V.multimodal_integrated_gradients(model, None, dataset, tok, divide_number=Dn, method=m,
                                                                           compounds=list(range(C))))[0])
        med = {m: float(np.median(v)) for m, v in t.items()}
        whole[str(C)] = {"ig_ms_per_compound": round(1e3 * med["ig"] / C, 3),
                         "smooth_ig_ms_per_compound": round(1e3 * med["smooth_ig"] / C, 3),
                         "ratio": round(med["smooth_ig"] / med["ig"], 3)}
        print("whole attribution C = %d: ig %.1f, smooth_ig %.1f ms per compound" % (C, 1e3 * med["ig"] / C, 1e3 * med["smooth_ig"] / C),
              flush=True)
    result["smooth_ig_vs_ig"] = whole
    V.multimodal_integrated_gradients(model, None, dataset, tok, divide_number=2, compounds=[0], batched=False, method="smooth_ig")
    t, _ = wall(lambda: V.multimodal_integrated_gradients(model, None, dataset, tok, divide_number=Dn, compounds=list(range(nl)),
                                                          batched=False, method="smooth_ig"))
    result["smooth_ig_loop"] = {"compounds": nl, "seconds": round(t, 4), "ms_per_compound": round(1e3 * t / nl, 3),
                                "batched_speedup": {C: round(1e3 * t / nl / whole[C]["smooth_ig_ms_per_compound"], 2) for C in whole}}
    print("smooth_ig loop: %.1f ms per compound" % (1e3 * t / nl), flush=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
