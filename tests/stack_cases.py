"""The layer lists, graphs and parameters of tests/test_gpu_stack_layers.py, with their fp64 reference (tests/stack_oracle.py).
tests/test_stack_oracle.py checks the relu margin of every case on the CPU, so a seed that does not meet it fails there and
never as a GPU mismatch.

Graphs are directed and irregular: a random size in 0..N per graph (at least one empty and one full-size graph per case),
about three stored entries per valid row (0..6, some rows without any) with signed values in +-[0.2, 0.8]; feature rows >= size
are zero.  Weights ~ N(0, 1/din); biases, beta and the moving mean ~ 0.2 N(0, 1); gamma and the moving variance in [0.5, 1.5].
A case's `graphs` / `data` entries name its deviations.
"""
import functools
import zlib

import numpy as np

import stack_oracle as S

_K = {"C": S.CONV, "D": S.DENSE, "B": S.NORM}
_A = {"n": S.ACT_NONE, "s": S.ACT_SIGMOID, "r": S.ACT_RELU, "t": S.ACT_TANH}
EPS = 1e-3

# name: T, N, layers ("Cr" = GraphConv + relu, ...), widths, sizes (the true sizes reach the kernels), gather, seed (chosen so
# that the relu margin holds: test_stack_oracle.test_relu_margin), graphs / data (deviations from the module docstring),
# bias (False: every matrix layer without one), dx (False: x does not require a gradient), routes (the routes that take it)
CASES = {
    "relu_chain": dict(T=40, N=10, layers="Cr Cr Dr", widths=(7, 24, 13, 64), sizes=False, gather=True, seed=0),
    "tanh_identity_per_node": dict(T=40, N=7, layers="Dt Cn Bt Ct", widths=(64, 16, 40, 40, 5), sizes=True, gather=False, seed=0),
    "norm_first_offset": dict(T=24, N=16, layers="Br Cs Dn", widths=(12, 12, 20, 6), sizes=True, gather=True, seed=0,
                              data="offset"),
    "two_norms_ragged_tile": dict(T=10, N=17, layers="Cr Bt Cs Bn Dt Dn", widths=(9, 33, 33, 20, 20, 8, 3), sizes=True,
                                  gather=True, seed=0),
    "eight_layers": dict(T=12, N=32, layers="Cr Bs Dt Cn Br Ct Ds Bn", widths=(5, 64, 64, 64, 33, 33, 20, 8, 8), sizes=True,
                         gather=True, seed=1, routes=(0, 1)),
    "one_node": dict(T=70, N=1, layers="Cr Dt", widths=(3, 9, 4), sizes=False, gather=True, seed=0, graphs="self_loop"),
    "narrow": dict(T=30, N=5, layers="Dn Cr Ds", widths=(1, 2, 3, 1), sizes=False, gather=True, seed=0),
    "no_bias_no_dx": dict(T=30, N=10, layers="Cs Dr", widths=(6, 16, 8), sizes=False, gather=True, seed=0, bias=False, dx=False),
    "dense32": dict(T=5, N=32, layers="Ct Cn", widths=(8, 8, 4), sizes=False, gather=True, seed=0, graphs="dense"),
    "dense32_duplicate": dict(T=5, N=32, layers="Ct Cn", widths=(8, 8, 4), sizes=False, gather=True, seed=0, graphs="dense_dup"),
    "second_trips_tiles": dict(T=520, N=32, layers="Cr Dt", widths=(3, 8, 4), sizes=True, gather=True, seed=4),
    "second_trips_one_graph": dict(T=1100, N=4, layers="Cr Dt", widths=(3, 8, 8), sizes=False, gather=True, seed=0),
}
# two small lists for the finite-difference check of the reference itself (tests/test_stack_oracle.py)
SMALL = {
    "fd_smooth": dict(T=3, N=4, layers="Ct Bs Dn", widths=(3, 4, 4, 2), sizes=True, gather=True, seed=0),
    "fd_relu": dict(T=3, N=4, layers="Cr Br Dr", widths=(3, 4, 4, 2), sizes=True, gather=False, seed=0),
}
# the module list of the layers.fused_stack test: not models.GCN's, true sizes, per-node output
MODULES = {
    "module_list": dict(T=40, N=10, layers="Cr Bt Dn", widths=(7, 12, 12, 5), sizes=True, gather=False, seed=0),
}
RELU_MARGIN = 1e-5


def _entry(case):
    for table in (CASES, SMALL, MODULES):
        if case in table:
            return table[case]
    raise KeyError(case)


def spec_of(case):
    c = _entry(case)
    names, w = c["layers"].split(), c["widths"]
    assert len(w) == len(names) + 1
    return tuple((_K[n[0]], _A[n[1]], w[l], w[l + 1], EPS if n[0] == "B" else 0.0) for l, n in enumerate(names))


def _graphs(rng, T, N, kind):
    """-> (sizes [T], adjs[t] = [(idx [n, 2] int64, val [n] float32, [N, N])])"""
    if kind in ("dense", "dense_dup"):
        # every row stores all N columns once: the longest row equals N and a graph holds N * N entries
        sizes = np.full(T, N)
        adjs = []
        for t in range(T):
            idx = np.stack(np.meshgrid(np.arange(N), np.arange(N), indexing="ij"), -1).reshape(-1, 2)
            val = rng.choice([-1.0, 1.0], N * N) * rng.uniform(0.2, 0.8, N * N) / N
            if kind == "dense_dup" and t == 3:
                # row 11 stores column 20 twice (N + 1 entries): both routes SUM duplicates, as the reference does
                at = 11 * N + 21
                idx = np.insert(idx, at, [11, 20], axis=0)
                val = np.insert(val, at, -0.4 / N)
            adjs.append([(idx.astype(np.int64), val.astype(np.float32), [N, N])])
        return sizes, adjs
    sizes = rng.integers(0, N + 1, T)
    sizes[rng.permutation(T)[:2]] = (0, N)               # one empty graph, one of full size
    adjs = []
    for t in range(T):
        rows, cols = [], []
        n = int(sizes[t])
        for r in range(n):
            if kind == "self_loop":
                k, c = 1, [r]
            else:
                k = min(n, int(rng.integers(0, 7)))
                c = rng.choice(n, k, replace=False)
            rows += [r] * k
            cols += list(c)
        if kind == "self_loop" and n and rng.random() < 0.3:
            rows, cols = [], []                          # a node without its self loop: a row without entries
        idx = np.array([rows, cols], np.int64).T.reshape(-1, 2)
        val = rng.choice([-1.0, 1.0], len(rows)) * rng.uniform(0.2, 0.8, len(rows))
        adjs.append([(idx, val.astype(np.float32), [N, N])])
    return sizes, adjs


@functools.lru_cache(maxsize=None)
def make_case(case):
    """-> dict of read-only float32 / integer arrays (what the kernels are given) and `ref`, the fp64 reference computed ONCE from
    exactly those values: spec, params, buffers, x, adjs, sizes (None unless the case hands the true sizes to the kernels),
    graph_sizes, gather, cotangent, ref."""
    c = _entry(case)
    rng = np.random.default_rng([c["seed"], zlib.crc32(case.encode())])     # the case's own stream, whatever else the tables hold
    T, N, spec = c["T"], c["N"], spec_of(case)
    graph_sizes, adjs = _graphs(rng, T, N, c.get("graphs"))
    valid = np.arange(N)[None, :] < graph_sizes[:, None]
    offset = c.get("data") == "offset"
    x = rng.standard_normal((T, N, spec[0][2])) + (4.0 if offset else 0.0)
    x = (x * valid[:, :, None]).astype(np.float32)
    params, buffers = [], []
    for kind, act, din, dout, eps in spec:
        if kind == S.NORM:
            params += [rng.uniform(0.5, 1.5, dout), 0.2 * rng.standard_normal(dout)]
            # offset data: the moving mean sits at the data's (4 + 0.1 N(0, 1)), so rstd (S1 - mean S0) cancels
            mean = 4.0 + 0.1 * rng.standard_normal(dout) if offset and not buffers else 0.2 * rng.standard_normal(dout)
            buffers.append((mean.astype(np.float32), rng.uniform(0.5, 1.5, dout).astype(np.float32)))
        else:
            w = rng.standard_normal((din, dout)) / np.sqrt(din)
            b = 0.2 * rng.standard_normal((1, dout) if kind == S.CONV else (dout,))
            params += [w, b if c.get("bias", True) else None]
            buffers.append(None)
    params = [None if p is None else p.astype(np.float32) for p in params]
    gather = c["gather"]
    cot = rng.standard_normal((T, spec[-1][3]) if gather else (T, N, spec[-1][3])).astype(np.float32)
    sizes = graph_sizes.astype(np.int32) if c["sizes"] else None
    ref = S.stack_reference(spec, params, buffers, x, adjs, sizes, gather, cot)
    for a in [x, cot, graph_sizes] + [p for p in params if p is not None] + [b for bb in buffers if bb for b in bb] + \
            ref["pre"] + ref["outs"] + [ref["out"], ref["dx"], ref["dparams"]] + [g for g in ref["grads"] if g is not None]:
        a.setflags(write=False)
    return dict(spec=spec, params=params, buffers=tuple(buffers), x=x, adjs=adjs, sizes=sizes, graph_sizes=graph_sizes,
                gather=gather, cotangent=cot, ref=ref, dx=c.get("dx", True), routes=c.get("routes", (0, 1, 2)))


def relu_margin_violations(case):
    """pre-activations of the case's relu layers that are neither exactly 0 (rows without entries, padded rows) nor at least
    RELU_MARGIN in magnitude -> [(layer, count, the smallest such magnitude)]"""
    d = make_case(case)
    bad = []
    for l, (kind, act, din, dout, eps) in enumerate(d["spec"]):
        if act != S.ACT_RELU:
            continue
        z = np.abs(d["ref"]["pre"][l])
        near = (z != 0) & (z < RELU_MARGIN)
        if near.any():
            bad.append((l, int(near.sum()), float(z[near].min())))
    return bad
