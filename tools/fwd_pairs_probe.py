#!/usr/bin/env python3
"""Per-phase cycle breakdown of graphconv_fwd_full_kernel, per ROLE (development tool, GPU box only).
The probe library is a build of the tree with fused.hip compiled with -DKGCN_PROBE.  A stamp reads the clock behind a wait for the
wave's LDS operations, so a probe build is slower than the product; the split between the phases is what it shows.
usage: KGCN_PROBE_LIB=build/variants/libkgcn_probe.so python tools/fwd_pairs_probe.py [graphs] [--normalize]"""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
out = os.environ.get("KGCN_PROBE_LIB", os.path.join(ROOT, "build", "variants", "libkgcn_probe.so"))
import kgcn_amd._lib as L
lib = ctypes.CDLL(out)
for name, (res, args) in L.SIGNATURES.items():
    getattr(lib, name).restype = res
    getattr(lib, name).argtypes = args
lib.kgcn_probe_set.argtypes = [ctypes.c_void_p]
from bench import make_cfg2
from kgcn_amd import ops
args = [a for a in sys.argv[1:] if not a.startswith("--")]
T = int(args[0]) if args else 100000
dev = torch.device("cuda:0")
wl = make_cfg2(T, dev, normalize=True) if "--normalize" in sys.argv else make_cfg2(T, dev)
csr = wl["csr"]
x, w = wl["x"], wl["w"]
bias = torch.zeros(64, device=dev)
y = torch.empty_like(x)
desc = ops._fused_adjacency(csr, False, T, 64, 64, False)
assert lib.kgcn_graphconv_fwd_pairs_route(T, 32, 64, 64, csr.padded4().max_nnz) == 1, "this batch does not take the pairs kernel"
probe = torch.zeros(2048 * 8, dtype=torch.int64, device=dev)
assert lib.kgcn_probe_set(ctypes.c_void_p(probe.data_ptr())) == 0
s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
p = lambda t: ctypes.c_void_p(t.data_ptr())
for rep in range(4):
    probe.zero_()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    rc = lib.kgcn_graphconv_fwd_f32(desc, p(x), p(w), p(bias), 64, 64, p(y), s)
    e1.record()
    torch.cuda.synchronize()
    assert rc == 0
pr = probe.cpu().numpy().reshape(2048, 8).astype(np.float64)
wave = np.arange(2048) % 8
role = wave >> 2
iters = T / 1024.0
print("%.1f us/launch (probe build); %.1f graphs per pair; cycles per graph (s_memtime ticks)" % (e0.elapsed_time(e1) * 1e3, iters))
names = {0: ["prologue", "land x(i), request x(i+1)", "land CSR(i), request CSR(i+1), slots(i+2)", "contraction", "store of the FW tile",
             "barrier wait", "last graph", "-"],
         1: ["prologue, first barrier", "aggregation, first scheduling scope (all eight passes as shipped)", "aggregation, second scope (four passes per scope)", "-", "-",
             "barrier wait", "last graph", "-"]}
for r in (0, 1):
    sel = pr[role == r]
    tot = sel.sum(1).mean() / iters
    print("wave %s: %.0f per graph" % ("R (reader / multiplier)" if r == 0 else "W (aggregator / writer)", tot))
    for k, n in enumerate(names[r]):
        if n == "-":
            continue
        v = sel[:, k].mean() / iters
        print("   %-66s %9.1f  (%4.1f%%)   min %.0f max %.0f over waves" % (n, v, 100 * v / tot, sel[:, k].min() / iters, sel[:, k].max() / iters))
