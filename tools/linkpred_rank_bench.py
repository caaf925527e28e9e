#!/usr/bin/env python3
"""The ranking stage of the link-prediction sample (run_enrichment.sh) at the sample's shape (N = 5,000, D = 128, cutoff
1,500,000 of 12,497,500 pairs; the label lists of tests/golden/g8_kg_linkpred.npz), one JSON line:
  fused      ops.pair_rank (select + emit) and ops.pair_rank_table: wall time of each call between device synchronisations
             (the calls synchronise themselves: CUDA events around them would not see the host part), the kernels' device
             times from a torch.profiler trace (the three histogram passes, the emit pass, the sort, the rest), the Gram
             passes' share of the fp32 MFMA peak (157.3 TFLOP/s; 2 D flop for each of the N (N - 1) / 2 pairs and pass), and
             the peak device memory beyond the inputs
  composed   the device path there was before: LinkPredictionNet.predict's GEMM -> torch.triu_indices -> gather -> torch.sort
             (descending) -> the first `cutoff`; the same clocks and the same memory figure
  host       the reference procedure on the host, from the [N, N] matrix: numpy lexsort over the 12.5 M (score, row, col)
             (timed once).  predscore.py itself builds and sorts a Python list of 12.5 M tuples and probes sets per entry; that
             takes minutes and is not worth timing in full, the lexsort is its floor
  agreement  the fused and the composed list name the same pairs, except pairs whose fp64 score lies within the two paths'
             rounding distance (D + 2) 2^-24 sum_k |h_ik h_jk| of the cutoff score
usage: python tools/linkpred_rank_bench.py [--steps K] [--warmup W] [--nodes N] [--cutoff C] [--skip-host] [--out profiles/linkpred_rank_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kgcn_amd import ops, predscore  # noqa: E402

MFMA_F32_TFLOPS = 157.3
dev = torch.device("cuda:0")


def wall(fn, steps, warmup):
    """median ms of fn() between device synchronisations, and its result."""
    for _ in range(warmup):
        out = fn()
    ts = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), out


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20


def kernel_times(fn, reps=3):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    groups = {"histogram_passes": 0.0, "emit_pass": 0.0, "pick": 0.0, "sort": 0.0, "unpack_mark_hits": 0.0, "other": 0.0}
    for ev in prof.key_averages():
        us = ev.device_time_total / reps
        if us <= 0:
            continue
        k = ev.key
        if "pair_tile_kernel" in k:
            groups["histogram_passes" if "ILi0E" in k or "<0>" in k else "emit_pass"] += us
        elif "pair_pick" in k:
            groups["pick"] += us
        elif "radix" in k or "sort" in k.lower() or "onesweep" in k.lower() or "histogram" in k.lower():
            groups["sort"] += us
        elif "pair_unpack" in k or "pair_mark" in k or "pair_hits" in k or "scan" in k.lower():
            groups["unpack_mark_hits"] += us
        else:
            groups["other"] += us
    return {k: round(v, 1) for k, v in groups.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nodes", type=int, default=5000)
    ap.add_argument("--cutoff", type=int, default=1500000)
    ap.add_argument("--skip-host", action="store_true", help="leave the host lexsort out (minutes beyond N = 5,000)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    N, D, cutoff = a.nodes, 128, a.cutoff
    rng = np.random.default_rng(0)
    hn = (rng.standard_normal((N, D)) * 0.1).astype(np.float32)
    h = torch.as_tensor(hn, device=dev)
    z = np.load(os.path.join(ROOT, "tests", "golden", "g8_kg_linkpred.npz"))
    keep = lambda ll: ll[:, (ll[0, :, 0] < N) & (ll[0, :, 2] < N) & (ll[0, :, 0] != ll[0, :, 2])]
    label_list, test_label_list = keep(z["label_list"]), keep(z["test_label_list"])
    test = predscore.label_pairs(test_label_list)
    target = predscore.label_pairs(np.concatenate([label_list[0], test_label_list[0]]))
    tc, sc = ops.pair_codes(target, dev), ops.pair_codes(test, dev)
    total = N * (N - 1) // 2
    ratios = predscore.top_ratios(total - (len(target) - len(test)))

    rank = lambda: ops.pair_rank(h, None, cutoff)
    rank_ms, (score, row, col) = wall(rank, a.steps, a.warmup)
    table = lambda: ops.pair_rank_table(score, row, col, tc, sc, ratios)
    table_ms, _ = wall(table, a.steps, a.warmup)
    both = lambda: (rank(), table())
    kt = kernel_times(both)
    flop = 2.0 * D * total
    fused = dict(pair_rank_ms=rank_ms, pair_rank_table_ms=table_ms, total_ms=rank_ms + table_ms, kernels_us=kt,
                 peak_mib=peak_mib(both),
                 gram_share_of_mfma_peak_histogram=flop * 3 / (kt["histogram_passes"] * 1e-6) / (MFMA_F32_TFLOPS * 1e12)
                 if kt["histogram_passes"] else None,
                 gram_share_of_mfma_peak_emit=flop / (kt["emit_pass"] * 1e-6) / (MFMA_F32_TFLOPS * 1e12) if kt["emit_pass"] else None)

    def composed():
        m = ops.dense(h, h.t().contiguous())                                   # LinkPredictionNet.predict
        idx = torch.triu_indices(N, N, 1, device=dev)
        s, order = torch.sort(m[idx[0], idx[1]], descending=True)
        order = order[:cutoff]
        return s[:cutoff], idx[0][order], idx[1][order]

    comp_ms, (cs, cr, cc) = wall(composed, a.steps, a.warmup)
    comp = dict(total_ms=comp_ms, peak_mib=peak_mib(composed))

    host = None
    if not a.skip_host:
        m = ops.dense(h, h.t().contiguous()).cpu().numpy()
        t0 = time.perf_counter()
        iu = np.triu_indices(N, 1)
        s = m[iu]
        order = np.lexsort((-iu[1], -iu[0], -s))[:cutoff]
        host = dict(lexsort_s=time.perf_counter() - t0, matrix_mib=m.nbytes / 2.0 ** 20,
                    note="numpy lexsort of all pairs from the [N, N] matrix; the reference's Python tuple sort and set probes are slower still")
        del m, s, order, iu

    fa = set((row.cpu().numpy().astype(np.int64) * N + col.cpu().numpy()).tolist())
    ca = set((cr.cpu().numpy().astype(np.int64) * N + cc.cpu().numpy()).tolist())
    diff = np.asarray(sorted(fa ^ ca), np.int64)
    cut = float(score[-1])
    worst = 0.0
    if len(diff):
        i, j = diff // N, diff % N
        h64 = hn.astype(np.float64)
        ref = np.einsum("pk,pk->p", h64[i], h64[j])
        tol = (D + 2) * 2.0 ** -24 * np.einsum("pk,pk->p", np.abs(h64[i]), np.abs(h64[j]))
        worst = float((np.abs(ref - cut) / tol).max())
    agreement = dict(pairs_in_one_list_only=int(len(diff)), worst_distance_from_cutoff_in_tol=worst, same_outside_rounding=worst <= 2.0)     # one tol for each path's rounding

    res = dict(N=N, D=D, cutoff=cutoff, pairs=total, fused=fused, composed=comp, host=host, agreement=agreement,
               device=torch.cuda.get_device_name(0))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
