#!/usr/bin/env python3
"""Integrated gradients of the protein-sequence CNN at the sample's shape: L = 1000 tokens, E = 25, D = 100 steps (101 copies),
models.SeqCNN at its real widths (505 / 200 / 100), for 1, 16 and 64 proteins.

  fused     visualization.seqcnn_integrated_gradients(fused=True): the bias-free first convolution and its window maxima once per
            protein, ops.conv1d_ig_expand over the copies, ops.conv1d_ig_reduce and one input-gradient pass (csrc/convig.hip).
  composed  fused=False: the scaled embedded rows as batch rows through the model's own first layer, autograd to them -- the only
            comparator, timed in the same run.
  loop      batched=False on --loop-proteins proteins: one batch-1 forward + backward per copy, the reference's loop.
  kernels   the two entry points alone at [C (D + 1), 250, 505] (--inner launches per timed window) against their algorithmic
            bytes -- C K T F floats written by expand (C T F read), 2 C K T F floats read by reduce (C T F written) -- and the
            8 TB/s HBM peak.

  accuracy  for information, both routes against the fp64 loop of tests/seqcnn_ig_oracle.py on this (unconditioned) model: protein 0
            at the full D, and 12 proteins at one and at four weighted copies.

Whole calls and kernels are timed with device events over --repeats runs after a warm-up of the same shapes, the two routes
alternating; reported are the median, the smallest and the largest run, and `spread_ms` = largest - smallest.  `fused_ahead` at a
protein count: the composed median exceeds the fused median by more than the larger of the two spreads.  `fused_default`, what
visualization.SEQCNN_IG_FUSED holds: fused_ahead at 16 AND at 64 proteins.  Prints one JSON line; --out writes it to a file too.

    python tools/seqcnn_ig_bench.py [--repeats 10] [--proteins 1 16 64] [--loop-proteins 1] [--out profiles/seqcnn_ig_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kgcn_amd import _lib, models, visualization as V  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=10)
ap.add_argument("--proteins", type=int, nargs="+", default=[1, 16, 64])
ap.add_argument("--loop-proteins", type=int, default=1)
ap.add_argument("--length", type=int, default=1000)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--inner", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda:0")
S, E, L, STEPS = 26, 25, args.length, args.steps
HBM_PEAK_GB_S = 8000.0
rng = np.random.default_rng(0)
G = max(args.proteins)
tokens = torch.as_tensor(rng.integers(0, S, (G, L)).astype(np.int32), device=dev)
torch.manual_seed(0)
model = models.SeqCNN(S, embedding_dim=E, label_dim=2).to(dev)
with torch.no_grad():
    model(None, None, sequences=tokens[:1])
    for conv in model.convs:                                   # biases away from their zero start, as after training
        conv.conv_bias.uniform_(-0.05, 0.05)


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
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4), "max_ms": round(float(np.max(ms)), 4),
            "spread_ms": round(float(np.max(ms) - np.min(ms)), 4)}


def call(n, **kw):
    return V.seqcnn_integrated_gradients(model, tokens, divide_number=STEPS, label_target=1, proteins=range(n), **kw)


result = {"length": L, "embedding_dim": E, "steps": STEPS, "widths": list(model.WIDTHS), "repeats": args.repeats,
          "rows_per_chunk": V.SEQCNN_IG_ROWS_PER_CHUNK, "device": torch.cuda.get_device_name(0),
          "timing": "device events around each call, the routes alternating; median, smallest and largest of `repeats` runs"}
ahead = {}
for n in args.proteins:
    ms_f, ms_c = timed([lambda: call(n, fused=True), lambda: call(n, fused=False)], args.repeats)
    a, b = call(n, fused=True), call(n, fused=False)
    big = max(float(np.abs(r["embedded_layer_IG"]).max()) for r in b)
    diff = max(float(np.abs(p["embedded_layer_IG"] - q["embedded_layer_IG"]).max()) for p, q in zip(a, b)) / big
    sf, sc = stats(ms_f), stats(ms_c)
    ahead[n] = bool(sc["median_ms"] - sf["median_ms"] > max(sf["spread_ms"], sc["spread_ms"]))
    result["proteins_%d" % n] = {"fused": sf, "composed": sc, "composed_over_fused": round(sc["median_ms"] / sf["median_ms"], 3),
                                 "fused_ahead": ahead[n], "IG_max_rel_diff_fused_vs_composed": diff}
# both routes against the fp64 per-copy loop of tests/seqcnn_ig_oracle.py on protein 0, for information: this model is untrained
# and not conditioned the way the cases of tests/test_gpu_seqcnn_ig.py are: its 101 copies hold some 7e7 relu and pool decisions, a
# handful of which fall on the other side of their threshold in fp32, so the figures are far above the tests' bounds
sys.path.insert(0, os.path.join(ROOT, "tests"))
import seqcnn_ig_oracle as IO  # noqa: E402
par = {"embeddings": model.embeddings, "w4": model.conv_out.conv_kernel, "b4": model.conv_out.conv_bias, "gamma1": model.bn1.gamma,
       "beta1": model.bn1.beta, "wh": model.hidden.kernel, "bh": model.hidden.bias, "gamma2": model.bn2.gamma, "beta2": model.bn2.beta,
       "wo": model.out.kernel, "bo": model.out.bias}
for i, conv in enumerate(model.convs, 1):
    par["w%d" % i], par["b%d" % i] = conv.conv_kernel, conv.conv_bias
par = {k: v.detach().cpu().numpy().reshape(-1) if k[0] in "bg" else v.detach().cpu().numpy() for k, v in par.items()}
table, tok_host = par["embeddings"].astype(np.float64), tokens.cpu().numpy()
ref = IO.integrated_gradients(par, table[tok_host[0]], [0.0, 1.0], "ig", STEPS)
big = float(np.abs(ref["ig"]).max())
result["accuracy_protein_0"] = {
    route: float(np.abs(call(1, fused=fused)[0]["embedded_layer_IG"] - ref["ig"]).max()) / big
    for route, fused in (("fused_vs_fp64", True), ("composed_vs_fp64", False))}
# ... and with few weighted copies, protein by protein: a run holds few enough decisions that most have none within rounding of
# its threshold; one that has shows the size of a single flipped first-layer unit (about 1 / sqrt(4 x 505) of an entry, over D)
few, ng = {}, min(12, G)
for method, D in (("grad_prod", 1), ("ig", 4)):
    got = [V.seqcnn_integrated_gradients(model, tokens, divide_number=D, method=method, label_target=1, proteins=range(ng), fused=f)
           for f in (True, False)]
    refs = [IO.integrated_gradients(par, table[tok_host[g]], [0.0, 1.0], method, D)["ig"] for g in range(ng)]
    few["%s_D%d" % (method, D)] = {
        route: [float("%.3e" % (np.abs(r["embedded_layer_IG"] - ref).max() / np.abs(ref).max())) for r, ref in zip(recs, refs)]
        for route, recs in zip(("fused_vs_fp64", "composed_vs_fp64"), got)}
result["accuracy_few_copies"] = few
nl = max(1, min(args.loop_proteins, G))
(ms_l,) = timed([lambda: call(nl, batched=False)], max(1, min(args.repeats, 3)))
result["loop"] = dict(stats(ms_l), proteins=nl, ms_per_protein=round(float(np.median(ms_l)) / nl, 3))

# the two kernels alone: the entry points themselves, --inner launches per timed window
C, K, T, F = min(16, G), STEPS + 1, L // 4, model.WIDTHS[0]
scales, weights = V.ig_scales("ig", STEPS)
Pm, bias = torch.randn((C, T, F), device=dev), torch.randn(F, device=dev) * 0.1
out, dout, r = torch.empty((C * K, T, F), device=dev), torch.randn((C * K, T, F), device=dev), torch.empty((C, T, F), device=dev)
al, wt = torch.tensor(scales, device=dev, dtype=torch.float32), torch.tensor(weights, device=dev, dtype=torch.float32)
ptr, stream = _lib.ptr, _lib.current_stream()


def expand():
    for _ in range(args.inner):
        _lib.check(_lib.lib.kgcn_ig_conv1d_expand_f32(ptr(Pm), C, K, T, F, ptr(al), ptr(bias), ptr(out), stream), "expand")


def reduce():
    for _ in range(args.inner):
        _lib.check(_lib.lib.kgcn_ig_conv1d_reduce_f32(ptr(dout), ptr(out), C, K, T, F, ptr(wt), ptr(r), stream), "reduce")


ms_e, ms_r = ([t / args.inner for t in ms] for ms in timed([expand, reduce], args.repeats))
n = C * T * F
eb, rb = 4 * (K * n + n), 4 * (2 * (K - 1) * n + n)          # the copy of weight 0 is not read
result["kernels"] = {"proteins": C, "rows": C * K, "launches_per_window": args.inner, "hbm_peak_gb_per_s": HBM_PEAK_GB_S}
for name, ms, nbytes in (("expand", ms_e, eb), ("reduce", ms_r, rb)):
    gbs = nbytes / np.median(ms) / 1e6
    result["kernels"][name] = dict(stats(ms), bytes=nbytes, gb_per_s=round(gbs, 1), fraction_of_peak=round(gbs / HBM_PEAK_GB_S, 3))
result["fused_default"] = bool(all(ahead.get(n, False) for n in (16, 64)))
result["module_constant"] = bool(V.SEQCNN_IG_FUSED)
line = json.dumps(result)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
