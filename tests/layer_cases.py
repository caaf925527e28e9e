"""The graphs, features and weights of tests/test_gpu_gat_maxpool.py, with their fp64 reference (oracle/kgcn_oracle.py: gat_fwd,
gat_bwd, graph_maxpool_fwd, graph_maxpool_bwd), computed ONCE per case.  tests/test_layer_cases.py proves on the CPU that every
case reaches the kernel branch it names and keeps the margins an fp32 kernel needs, so a bad seed fails there and never as a GPU
mismatch.

A case is T graphs of N padded nodes (rect: M rows x K columns) with C adjacency channels of DIFFERENT structure:
  * true size 0..N per graph, at least one empty and one full-size graph; feature rows at or behind the size are zero, padded rows
    store nothing and nothing refers to them
  * entries are directed (a row prefers columns whose reverse entry is not stored), values signed in +-[0.2, 0.8]
  * features ~ N(0, 1) pushed away from 0: |x| >= 0.05 on valid rows
  * FULL ROWS, in graphs of size N only: row 1 + c of channel c stores every column (e - s == K for the padded shape), the row
    behind it all columns but one (exactly one implicit zero).  Their values have the sign -sign(x[col, 0]): every product of
    feature 0 is negative, so the full row's maximum is negative and the neighbour's is its implicit zero
  * SINKS, in about one (graph, channel) of four (narrow: one of seven) and in one full-size graph: a valid node that stores nothing while row 0 and one
    more row (in a full-size graph also the full row and its neighbour) refer to it; every other valid row stores 1..6 entries.  GAT gathers denom = 0 there: alpha = E / 1e-10 ~ 1e10, the
    sigmoid saturates to exactly 0 or 1
  * the FAINT sink (the first sink of channel 0, where D >= 2 C): the features of the sink s and of row 0 are solved so that
    u[s] = v[0] = u[0] = v[s] = t / 2 with t ~ -125.  The entry (0, s) then has E = exp(0.2 t) ~ 1e-11 and
    alpha = E / (0 + 1e-10) ~ 0.1 with |alpha x[s]| <= FAINT_R: the ONE place where the constant 1e-10 decides an output that
    is not saturated (and a gradient that is not 0).  These two nodes' features are large (|x| ~ 1e2), so max-pooling, whose
    tolerance is absolute, gets the features without them
  * a HUB row of 66 entries (longer than a wave) in the full-size graph of the N = 70 case
  * a second, GRID-valued data set on the same structure for max-pooling: features in {-1, -0.5, 0, 0.5, 1}, values in
    {+-0.5, +-1}, so that ties -- among entries, with implicit zeros, inside full rows -- really occur; it is judged against the
    fp32 form of the oracle (exact tie sets)
weight_a ~ N(0, 1) * T_STD / sqrt(2 D): the scores t = u[col] + v[row] have a standard deviation of about T_STD.
"""
import functools
import zlib

import numpy as np

from oracle import kgcn_oracle as K

T_STD = 1.0
FAINT_R = 1.5                    # the largest |alpha x| of the faint entry: sigmoid'(r) r is largest near 1.5
HUB_LEN = 66
SINK_SHARE = 0.25

# name: T, N, D, C, seed (chosen so that tests/test_layer_cases.py holds: margins, saturation cap, one-way share),
# sinks (share of (graph, channel)s with a sink, default SINK_SHARE); the comment above a case: what it reaches.
# `rules_out`: the wrong variants of tests/test_layer_cases.py that the case tells from the reference by >= 100 x the GPU tolerance:
#   a = max-pooling that always admits the implicit zero, b = the gradient on the transposed structure,
#   c = GAT's denominator gathered at the row, d = GAT's 1e-10 replaced by 1e-6
# The GPU test runs on the tolerances the older tests write, none widened; test_layer_cases.test_fp32_oracle_distance prints how far
# the numpy fp32 oracle is from the fp64 one per case (out <= 1.9e-6, dx <= 4.3e-6 of 7.1, dweight_a <= 6.6e-5 of 27).
CASES = {
    # 4-lane groups, odd N, 259 nodes (< 512 workgroups of gat_bwd_dots), two channels (beta = 1 accumulation)
    # D < 2 C: no faint sink, every sink saturates, d cannot show.  sinks: at 0.25 the two rows that refer to a sink are 10 - 20 %
    # of the ~ 3.5 valid rows of a graph, the whole saturation cap
    "narrow": dict(T=37, N=7, D=3, C=2, seed=3, sinks=0.15, rules_out="abc"),
    # 1-lane groups; N = 1: a self loop is a full row, a missing one an empty row.  Row == column and no second node:
    # b, c and d cannot show
    "one_node": dict(T=70, N=1, D=1, C=1, seed=0, rules_out="a"),
    # 64-lane groups with a one-column second trip; 520 nodes: npb = 2, 260 workgroups
    "wave_plus_one": dict(T=40, N=13, D=65, C=1, seed=0, rules_out="abcd"),
    # 512 nodes: npb = 1 at the cap; an even width that is no multiple of 4
    "exactly_512": dict(T=32, N=16, D=50, C=1, seed=0, rules_out="abcd"),
    # 513 nodes: npb = 2, 257 workgroups, the last one holds ONE node
    "short_last_block": dict(T=27, N=19, D=8, C=2, seed=0, rules_out="abcd"),
    # N > 64, the 66-entry row, 70-entry full rows
    "hub": dict(T=3, N=70, D=16, C=1, seed=0, rules_out="abcd"),
    # second 256-column trip of gat_bwd_dots_kernel; N just above 32
    "wide": dict(T=8, N=33, D=260, C=1, seed=0, rules_out="abcd"),
    # M != K in both max-pooling kernels (through ops.graph_maxpool; no GAT: it wants a square adjacency).  The transposed
    # structure has another shape: b does not apply
    "rect": dict(T=9, N=5, K=9, D=6, C=1, seed=0, gat=False, rules_out="a"),
}


def _columns(rng, r, nk, k, have, sink):
    """k distinct columns of row r, never the sink (the rows that refer to it are chosen, not drawn); columns j whose reverse
    (j, r) is stored, and r itself, come last (nine rows of ten)"""
    perm = [int(j) for j in rng.permutation(nk) if j != sink]
    if rng.random() >= 0.1:
        perm = [j for j in perm if j != r and (j, r) not in have] + [j for j in perm if j == r or (j, r) in have]
    return perm[:k]


def _structure(rng, T, M, K_, C, hub, sink_share):
    """-> rsizes [T], csizes [T], rows[t][c] = {row: [columns]}, full[(t, c)] = (full row, neighbour or None),
    sinks[(t, c)] = (sink, the second row that refers to it), hubs[(t, c)] = row"""
    rs = rng.integers(0, M + 1, T)
    forced = rng.permutation(T)[:2]
    rs[forced] = (0, M)
    if T == 3:                                            # the hub case: the third graph is large enough for a sink
        rs[[t for t in range(3) if t not in forced]] = rng.integers(3, M + 1)
    cs = np.where(rs > 0, rs + (K_ - M), 0)
    rows, full, sinks, hubs = [], {}, {}, {}
    for t in range(T):
        n, nk = int(rs[t]), int(cs[t])
        per_ch = []
        for c in range(C):
            special = {}
            if n == M:
                fr = (1 + c) % M
                nb = fr + 1 if fr + 1 < M and M >= 3 else None
                full[(t, c)] = (fr, nb)
                special[fr] = "full"
                if nb is not None:
                    special[nb] = "neighbour"
                if hub:
                    hubs[(t, c)] = 4
                    special[4] = "hub"
            s = o = None
            if M == K_ and n >= 3 and (rng.random() < sink_share or t == forced[1]):
                cand = [r for r in range(1, n) if r not in special]
                if cand:
                    s = int(rng.choice(cand))
                    others = [r for r in range(1, n) if r != s and r not in special] or [r for r in range(1, n) if r != s]
                    o = int(rng.choice(others))
                    sinks[(t, c)] = (s, o)
            have, g = set(), {}
            for r in range(n):
                kind = special.get(r)
                if r == s:
                    cols = []
                elif M == 1:                                # one node: the self loop or nothing (never in the forced full graph)
                    cols = [] if (t != forced[1] and rng.random() < 0.35) else [0]
                elif kind == "full":
                    cols = list(range(nk))
                elif kind == "neighbour":
                    drop = int(rng.integers(0, nk))
                    cols = [j for j in range(nk) if j != drop]
                elif kind == "hub":
                    cols = sorted(int(j) for j in rng.choice(nk, HUB_LEN, replace=False))
                else:
                    k = 1 + int(rng.choice(6, p=[0.3, 0.25, 0.2, 0.1, 0.1, 0.05]))
                    cols = _columns(rng, r, nk, min(k, nk), have, s)
                    if s is not None and r in (0, o) and s not in cols:
                        cols[-1] = s
                    cols = sorted(cols)
                g[r] = cols
                have.update((r, j) for j in cols)
            per_ch.append(g)
        rows.append(per_ch)
    if M == 1:
        for t in range(T):
            if rows[t][0].get(0) == []:
                full.pop((t, 0), None)
    return rs, cs, rows, full, sinks, hubs


def _adjs(rng, rows, full, x, M, K_, grid):
    """COO triples of the structure with values drawn for the data set `x` (full rows and their neighbours: -sign(x[col, 0]))"""
    out = []
    for t, per_ch in enumerate(rows):
        chans = []
        for c, g in enumerate(per_ch):
            idx = np.array([(r, j) for r in sorted(g) for j in g[r]], np.int64).reshape(-1, 2)
            n = len(idx)
            mag = rng.choice([0.5, 1.0], n) if grid else rng.uniform(0.2, 0.8, n)
            sign = rng.choice([-1.0, 1.0], n)
            for r in full.get((t, c), ()):
                if r is None:
                    continue
                sel = idx[:, 0] == r
                sx = -np.sign(x[t, idx[sel, 1], 0])
                sign[sel] = np.where(sx != 0, sx, sign[sel])
            chans.append((idx, (sign * mag).astype(np.float32), [M, K_]))
        out.append(chans)
    return out


def _solve_faint(x, weight_a, nodes, D):
    """features of `nodes` with u = x . wa[:D] = v = x . wa[D:] = t / 2 for channel 0 and = -2 for every other channel (least
    norm: no score of these nodes is large and positive in any channel), pushed to |x| >= 0.05; t < 0 such that
    alpha max|x| = exp(0.2 t) / 1e-10 max|x| = FAINT_R (a fixed point: the features grow with |t|)"""
    A = np.concatenate([np.stack([w[:D, 0], w[D:, 0]]) for w in weight_a]).astype(np.float64)
    P = A.T @ np.linalg.inv(A @ A.T)
    rest = np.full(len(A) - 2, -2.0)
    t = 5.0 * np.log(1.0e-10)
    for _ in range(8):
        sol = P @ np.concatenate([[t / 2, t / 2], rest])
        t = 5.0 * np.log(1.0e-10 * FAINT_R / np.abs(sol).max())
    sol = np.where(np.abs(sol) < 0.05, np.where(sol < 0, -0.05, 0.05), sol)
    for g, j in nodes:
        x[g, j] = sol


@functools.lru_cache(maxsize=None)
def make_case(case):
    """-> dict of read-only arrays: what the kernels are given (float32 / integers) and the reference computed from exactly
    those values.  x, adjs: the generic data (x_pool: what max-pooling gets, x without the faint sink's two solved rows; the
    full rows' signs follow x_pool); xg, adjs_grid: the grid data (same structure); weight_a [C][2 D, 1]; g: the
    cotangent [T, M, D]; ref: gat_out, gat_dx, gat_dwa (fp64), mp_out, mp_dx (fp64, generic), mpg_out, mpg_dx (fp32, grid)."""
    c = CASES[case]
    rng = np.random.default_rng([c["seed"], zlib.crc32(case.encode())])
    T, M, D, C = c["T"], c["N"], c["D"], c["C"]
    K_ = c.get("K", M)
    gat = c.get("gat", True)
    rs, cs, rows, full, sinks, hubs = _structure(rng, T, M, K_, C, hub=(case == "hub"), sink_share=c.get("sinks", SINK_SHARE))
    valid = (np.arange(K_)[None, :] < cs[:, None])[:, :, None]
    z = rng.standard_normal((T, K_, D))
    x = z + 0.05 * np.where(z < 0, -1.0, 1.0)
    wa = [(rng.standard_normal((2 * D, 1)) * T_STD / np.sqrt(2 * D)).astype(np.float32) for _ in range(C)]
    x_pool = (x * valid).astype(np.float32)              # max-pooling: without the faint sink's large features
    faint = None
    if gat and D >= 2 * C:                               # narrow: 4 conditions on 3 features
        faint = min((k for k in sinks if k[1] == 0), default=None)
        if faint is not None:
            _solve_faint(x, wa, [(faint[0], sinks[faint][0]), (faint[0], 0)], D)
    x = (x * valid).astype(np.float32)
    xg = (rng.integers(-2, 3, size=(T, K_, D)) * 0.5 * valid).astype(np.float32)
    adjs = _adjs(rng, rows, full, x_pool, M, K_, grid=False)
    adjs_grid = _adjs(rng, rows, full, xg, M, K_, grid=True)
    g = rng.standard_normal((T, M, D)).astype(np.float32)
    ref = {}
    with np.errstate(over="ignore"):                     # sigmoid(-1e10): exp overflows to inf, 1 / inf = 0 is the value meant
        if gat:
            ref["gat_out"] = K.gat_fwd(x, adjs, wa)
            ref["gat_dx"], dwa = K.gat_bwd(x, adjs, wa, g)
            ref["gat_dwa"] = tuple(dwa)
    ref["mp_out"] = K.graph_maxpool_fwd(x_pool, adjs)
    ref["mp_dx"] = K.graph_maxpool_bwd(x_pool, adjs, g)
    ref["mpg_out"] = K.graph_maxpool_fwd(xg, adjs_grid, dtype=np.float32)
    ref["mpg_dx"] = K.graph_maxpool_bwd(xg, adjs_grid, g, dtype=np.float32)
    for a in [x, x_pool, xg, g, rs, cs] + wa + [m[i] for aa in (adjs, adjs_grid) for chans in aa for m in chans for i in (0, 1)] + \
            [v for v in ref.values() if isinstance(v, np.ndarray)] + list(ref.get("gat_dwa", ())):
        a.setflags(write=False)
    return dict(T=T, M=M, K=K_, D=D, C=C, gat=gat, sizes=rs, col_sizes=cs, x=x, x_pool=x_pool, xg=xg, adjs=adjs, adjs_grid=adjs_grid,
                weight_a=tuple(wa), g=g, ref=ref, full=full, sinks=sinks, hubs=hubs, faint=faint, rules_out=c["rules_out"])
