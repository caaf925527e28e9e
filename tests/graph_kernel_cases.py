"""The cases of tests/test_gpu_graph_kernel_ops.py: inputs for every op of kgcn_amd/csrc/graphkern.hip on its own, beyond the 13
nodes and 100 graphs of tests/test_gpu_graph_kernel.py, each with the result a plain reference gives.  The references below are
numpy and Python integers only and share no code with kgcn_amd; the Weisfeiler-Lehman partitions and Grams of the graph set come
from tests/graph_kernel_oracle.py.  Everything is an integer: the GPU tests compare with assert_array_equal and choose no tolerance.
tests/test_graph_kernel_cases.py proves on the CPU that every case has the property it is named for.

References
  ref_sorted_nbr(entries, num_nodes, colours)   the stored entries' colours, ascending within a row, rows in CSR order; and the
                                                class of (own colour, that list) of every row that exists
  ref_wl_runs(colours, num_nodes, offset)       (run_ptr, col, graph, count): graphs in order, columns ascending within a graph
  ref_sp_runs(entries, num_nodes, labels, directed)   the same for the keys label_k << 20 | label_j << 8 | distance
  ref_gram(col, graph, count, G)                int64 K by np.add.at into a dense count matrix, (columns, diag_columns, dense_columns)
Entries are (graph, row, col) arrays of the STORED entries.  An entry whose column is no node of its graph (num_nodes <= col < M)
is what the two kernels treat differently, and the references say how: ref_sp_runs ignores it, ref_sorted_nbr gives it the colour
the colour array holds there, -1.

Families
  gram      GRAM_NAMES: synthetic runs handed to ops.gram_from_runs in a seeded shuffle.  G of 1, 64, 65, 128, 129, 193, 260 (one
            to five tile rows of 64: 260 gives the 15 workgroups with every tj - ti of 0..4), each with chunk_cols 16 and the
            default 1,024; dense column counts of 0, 1, 15, 16, 17, 33, 50 against 16 and of 1023, 1024, 1025, 2500 against 1,024;
            column pairs that differ in bit 63, bit 32 and bit 0 alone; graphs without a run, from three tile rows on one whole
            tile row of them; counts up to 2^20 in three columns, so K passes 2^32 and (asserted here) stays below 2^53.
  wl runs   WL_RUNS_M: colours [T, M] for M of 1, 255, 256, 257, 1000, 4096 (emit_runs' segments are (n + 255) / 256 long), graphs
            of M, M - 1, 1 and 0 nodes; three colour values (runs far longer than a segment), all distinct, all equal; values up
            to 2^31 - 2; rows that do not exist hold PAD_JUNK, which must not be read.
  wl set    wl_set(): 200 sparse random graphs of 40..300 nodes with two labels, two stars of 299 leaves that differ in the
            label of the LAST leaf only, K_24, a graph with every edge three times, two triangles and a hexagon, a graph of 0 and
            one of 1 node: 62,400 rows at M = 300 for the radix sort and the scan of wl_rank.
  refine    wl_direct(): a CSR that is not symmetric, with repeated entries, entries in rows that do not exist and entries whose
            column is no node; two rows of 280 entries equal in their first 256 and different after; a row pair that differs in
            one out-of-graph entry alone.
  sp        SP_NAMES: one batch at M = 128 with n of 0, 1, 2, 3, 16, 17, 23, 64, 90, 91, 127, 128 (paths up to distance 127,
            cycles, a star, a complete graph, two components, isolated nodes, tripled edges); M == n for M of 1, 2, 3, 16, 17 (the
            part and dist arrays sit right behind the n^2 keys); 32 paths of 128 nodes with 4,096 distinct labels and a 33rd graph
            of 100 nodes in two components, all of rank 4,095, so that rank meets real distances and 255 -- the key 0xffffffff,
            5,000 times beside the 6,384 padding keys of the bitonic network, which are the same number; one directed CSR with
            out-of-graph columns and a one-way path.

The references of all 31 cases together build in 1.2 to 1.6 s (tests/test_graph_kernel_cases.py prints the figure and holds it
under 30 s); the largest part is the two oracle passes over the wl set."""
import functools
import zlib
from collections import namedtuple

import numpy as np

import graph_kernel_oracle as O

PAD_JUNK = 77                      # what colour / label rows that do not exist hold where the op must not read them
TILE = 64                          # kTile of graphkern.hip
DEFAULT_CHUNK = 1024               # ops.GRAM_CHUNK_COLS


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


# ---- references ------------------------------------------------------------------------------------------------------------------
def ref_sorted_nbr(entries, num_nodes, colours):
    """-> (sorted_nbr [nnz] int32: per row of the CSR (graph, then row) the colours of its stored columns, ascending;
    classes [T, M] int64: the id of the class of (own colour, that list) for every row that exists, -1 elsewhere)."""
    g, r, c = (np.asarray(a, np.int64) for a in entries)
    colours = np.asarray(colours)
    T, M = colours.shape
    lists = {}
    for gi, ri, ci in zip(g.tolist(), r.tolist(), c.tolist()):
        lists.setdefault((gi, ri), []).append(int(colours[gi, ci]))
    out = []
    for key in sorted(lists):
        out.extend(sorted(lists[key]))
    ids, classes = {}, np.full((T, M), -1, np.int64)
    for t in range(T):
        for v in range(int(num_nodes[t])):
            sig = (int(colours[t, v]), tuple(sorted(lists.get((t, v), []))))
            classes[t, v] = ids.setdefault(sig, len(ids))
    return np.array(out, np.int32), classes


def _runs(per_graph):
    """per graph (ascending uint64 columns, counts) -> (run_ptr int64 [T + 1], col int64 holding the u64 bits, graph, count int32)"""
    ptr = np.zeros(len(per_graph) + 1, np.int64)
    ptr[1:] = np.cumsum([len(v) for v, _ in per_graph])
    col = np.concatenate([v for v, _ in per_graph] + [np.zeros(0, np.uint64)]).astype(np.uint64).view(np.int64)
    graph = np.concatenate([np.full(len(v), t, np.int32) for t, (v, _) in enumerate(per_graph)] + [np.zeros(0, np.int32)])
    count = np.concatenate([n for _, n in per_graph] + [np.zeros(0, np.int64)]).astype(np.int32)
    return ptr, col, graph, count


def ref_wl_runs(colours, num_nodes, offset):
    colours = np.asarray(colours)
    per = []
    for t in range(colours.shape[0]):
        vals, cnt = np.unique(colours[t, :int(num_nodes[t])].astype(np.int64), return_counts=True)
        per.append((vals.astype(np.uint64) + np.uint64(offset), cnt))
    return _runs(per)


def ref_sp_runs(entries, num_nodes, labels, directed):
    """Breadth-first levels of all sources at once: the frontier matrix times the 0/1 adjacency (float32 holds these sums of at most
    128 ones exactly).  directed: a stored entry leads from its row to its column only; otherwise both ways.  Entries that name a
    row or a column at or past num_nodes change nothing.  Unreachable pairs get the distance 255."""
    g, r, c = (np.asarray(a, np.int64) for a in entries)
    labels = np.asarray(labels)
    per = []
    for t in range(labels.shape[0]):
        n = int(num_nodes[t])
        sel = (g == t) & (r < n) & (c < n)
        adj = np.zeros((n, n), np.float32)
        adj[r[sel], c[sel]] = 1.0
        if not directed:
            adj[c[sel], r[sel]] = 1.0
        reach = np.eye(n, dtype=bool)
        dist = np.where(reach, 0, 255).astype(np.int64)
        frontier, d = reach, 0
        while frontier.any():
            d += 1
            frontier = (frontier.astype(np.float32) @ adj > 0) & ~reach
            dist[frontier] = d
            reach = reach | frontier
        lab = labels[t, :n].astype(np.int64)
        keys = (lab[:, None] << 20 | lab[None, :] << 8 | dist).reshape(-1)
        vals, cnt = np.unique(keys, return_counts=True)
        per.append((vals.astype(np.uint64), cnt))
    return _runs(per)


def ref_gram(col, graph, count, G):
    """-> (K [G, G] int64, (columns, diag_columns, dense_columns)): a column is a distinct value of the u64 bits; one that occurs in a
    single run is a diag column."""
    keys = np.ascontiguousarray(col).view(np.uint64)
    uniq, inv = np.unique(keys, return_inverse=True)
    inv = inv.reshape(-1)
    F = np.zeros((G, max(len(uniq), 1)), np.int64)
    np.add.at(F, (np.asarray(graph, np.int64), inv), np.asarray(count, np.int64))
    assert (F.astype(np.float64) ** 2).sum(1).max(initial=0.0) < 2.0 ** 62                # the int64 products below cannot wrap
    K = F @ F.T
    occ = np.bincount(inv, minlength=len(uniq))
    diag = int((occ == 1).sum())
    return K, (int(len(uniq)), diag, int(len(uniq)) - diag)


# ---- Gram from synthetic runs ----------------------------------------------------------------------------------------------------
GramSpec = namedtuple("GramSpec", "G chunk_cols dense")            # chunk_cols None: the default
GRAM_SPECS = {"g%d_c%s_d%d" % (G, "def" if cc is None else cc, d): GramSpec(G, cc, d) for G, cc, d in (
    (1, 16, 0), (64, 16, 1), (65, 16, 15), (128, 16, 16), (129, 16, 17), (193, 16, 33), (260, 16, 50), (260, 16, 0),
    (1, None, 0), (64, None, 1023), (65, None, 1024), (128, None, 1025), (129, None, 2500), (193, None, 1024), (260, None, 1025))}
GRAM_NAMES = list(GRAM_SPECS)
BIT_PAIRS = (63, 32, 0)
GramCase = namedtuple("GramCase", "name spec col graph count empty K stats")


def gram_empty_graphs(G):
    """the graphs of a case that get no run: two scattered ones, and from three tile rows on the whole tile row before the last
    full one (the last graph always has runs, so a last tile of one graph is a live one)"""
    if G < 8:
        return []
    tiles = -(-G // TILE)
    empty = {5, min(G - 2, TILE - 1)}
    if tiles >= 3:
        row = 1 if tiles < 5 else 3
        empty |= set(range(row * TILE, (row + 1) * TILE))
    return sorted(empty)


@functools.lru_cache(maxsize=None)
def gram_case(name):
    spec, rng = GRAM_SPECS[name], _rng(name)
    G, dense = spec.G, spec.dense
    empty = gram_empty_graphs(G)
    live = np.array(sorted(set(range(G)) - set(empty)), np.int64)
    assert dense == 0 or len(live) >= 2
    ndiag = len(live) + 8
    values = rng.integers(0, 2 ** 64, dense + ndiag, dtype=np.uint64)
    for k, bit in enumerate(BIT_PAIRS):
        values[2 * k + 1] = values[2 * k] ^ np.uint64(1 << bit)
    assert len(np.unique(values)) == len(values)
    values = values[rng.permutation(len(values))]
    cols, graphs = [], []
    for k in range(dense):                                          # the first dense column: every live graph, so every tile pair
        members = live if k == 0 else rng.choice(live, int(rng.integers(2, len(live) + 1)), replace=False)
        cols.append(np.full(len(members), values[k]))
        graphs.append(members)
    for k in range(ndiag):                                          # every live graph has a column of its own
        cols.append(values[dense + k:dense + k + 1])
        graphs.append(live[k:k + 1] if k < len(live) else rng.choice(live, 1))
    col, graph = np.concatenate(cols), np.concatenate(graphs).astype(np.int32)
    count = rng.integers(1, 51, len(col)).astype(np.int64)
    big = [values[dense]] + [values[k] for k in (0, dense // 2) if k < dense]           # one diag column, up to two dense ones
    sel = np.isin(col, np.array(big, np.uint64))
    count[sel] = rng.integers(2 ** 19, 2 ** 20 + 1, int(sel.sum()))
    count[np.flatnonzero(sel)[0]] = 2 ** 20
    order = rng.permutation(len(col))                               # sorted by neither column nor graph
    col, graph, count = col[order].view(np.int64), graph[order], count[order].astype(np.int32)
    assert len(set(zip(col.tolist(), graph.tolist()))) == len(col)                      # the documented shape of the runs
    K, stats = ref_gram(col, graph, count, G)
    assert 2 ** 32 < K.max() < 2 ** 53                              # the kernel's stated precondition
    for a in (col, graph, count, K):
        a.setflags(write=False)
    return GramCase(name, spec, col, graph, count, tuple(empty), K, stats)


# ---- wl_runs on synthetic colours ------------------------------------------------------------------------------------------------
WL_RUNS_M = (1, 255, 256, 257, 1000, 4096)
WL_RUNS_T = {1: 3, 255: 4, 256: 5, 257: 4, 1000: 5, 4096: 5}
WL_RUNS_OFFSET = 3 << 32
WL_RUNS_PATTERNS = ("three", "distinct", "equal", "big", "three")
MAX_COLOUR = 2 ** 31 - 2
WlRunsCase = namedtuple("WlRunsCase", "M T num_nodes colours patterns runs")


@functools.lru_cache(maxsize=None)
def wl_runs_case(M):
    rng, T = _rng("wl_runs_%d" % M), WL_RUNS_T[M]
    num_nodes = np.array([M, M - 1, M, 1, 0][:T], np.int32)
    colours = np.full((T, M), PAD_JUNK, np.int32)
    for t in range(T):
        n, pattern = int(num_nodes[t]), WL_RUNS_PATTERNS[t]
        if pattern == "three":
            row = rng.choice([0, 7, MAX_COLOUR], n)
        elif pattern == "distinct":
            row = rng.choice(MAX_COLOUR, n, replace=False)          # 0 .. 2^31 - 3, and the largest value below
            if n:
                row[int(rng.integers(n))] = MAX_COLOUR
        elif pattern == "equal":
            row = np.full(n, 5)
        else:
            row = rng.integers(MAX_COLOUR - 40, MAX_COLOUR + 1, n)
        colours[t, :n] = row
    runs = ref_wl_runs(colours, num_nodes, WL_RUNS_OFFSET)
    for a in (colours, num_nodes) + runs:
        a.setflags(write=False)
    return WlRunsCase(M, T, num_nodes, colours, WL_RUNS_PATTERNS[:T], runs)


# ---- the graph set of the refinement and the ranking -----------------------------------------------------------------------------
WL_M = 300
WL_ITERATIONS = 3
WL_NAMED = ("star_a", "star_b", "k24", "tripled", "triangles", "hexagon", "none", "one")
WlSet = namedtuple("WlSet", "graphs index colours gram columns")


def _random_graph(rng, n, edges, labels=2):
    a, b = rng.integers(0, n, edges), rng.integers(0, n, edges)
    keep = a != b
    pairs = np.stack([np.maximum(a, b)[keep], np.minimum(a, b)[keep]], 1)                 # a repeated pair is a multi-edge
    return n, O.both_ways(pairs), rng.integers(0, labels, n).astype(np.int64)


def _star(n, last_label):
    lab = np.zeros(n, np.int64)
    lab[n - 1] = last_label
    return n, O.both_ways([(i, 0) for i in range(1, n)]), lab


@functools.lru_cache(maxsize=None)
def wl_graphs():
    rng = _rng("wl_set")
    graphs = []
    for _ in range(200):
        n = int(rng.integers(40, WL_M + 1))
        graphs.append(_random_graph(rng, n, int(rng.integers(n // 2, 2 * n))))
    zeros = lambda n: np.zeros(n, np.int64)  # noqa: E731
    n3, e3, l3 = _random_graph(rng, 30, 45)
    named = {"star_a": _star(WL_M, 0), "star_b": _star(WL_M, 1),   # centre rows of 299 entries that differ in the last one alone
             "k24": (24, O.both_ways([(i, j) for i in range(24) for j in range(i)]), zeros(24)),
             "tripled": (n3, np.concatenate([e3, e3, e3]), l3),
             "triangles": (6, O.both_ways(O.cycle(3) + O.cycle(3, 3)), zeros(6)),
             "hexagon": (6, O.both_ways(O.cycle(6)), zeros(6)),
             "none": (0, np.zeros((0, 2), np.int64), zeros(0)),
             "one": (1, np.zeros((0, 2), np.int64), zeros(1))}
    index = {}
    for name in WL_NAMED:
        index[name] = len(graphs)
        graphs.append(named[name])
    return tuple(graphs), index


@functools.lru_cache(maxsize=None)
def wl_set():
    """graphs, the index of the named ones, the oracle's colours after every iteration, its Gram and (columns, diag, dense)"""
    graphs, index = wl_graphs()
    colours = O.wl_colours(list(graphs), WL_ITERATIONS)
    F = O.wl_features(list(graphs), WL_ITERATIONS)
    occ = np.asarray((F > 0).sum(0)).reshape(-1)
    columns = (int((occ > 0).sum()), int((occ == 1).sum()), int((occ > 1).sum()))
    assert columns[1] > 0 and columns[2] > 0                       # both halves of the Gram have work
    return WlSet(graphs, index, colours, O.gram(F), columns)


def max_degree(graph):
    n, e, _ = graph
    return max([len(x) for x in O.neighbours(n, e)] + [0])


# ---- wl_refine on a CSR that is not symmetric -----------------------------------------------------------------------------------
WlDirect = namedtuple("WlDirect", "T M num_nodes colours entries sorted_nbr classes long_rows pad_rows")


@functools.lru_cache(maxsize=None)
def wl_direct():
    rng, T, M = _rng("wl_direct"), 6, 40
    num_nodes = np.array([40, 33, 0, 1, 40, 20], np.int32)
    colours = np.full((T, M), -1, np.int32)
    for t in range(T):
        colours[t, :num_nodes[t]] = rng.integers(0, 4, num_nodes[t])
    colours[0, 3] = colours[0, 7] = 2
    colours[4] = colours[0]                                        # the long rows (0, 3) and (4, 7) have one own colour
    colours[5, 0] = colours[5, 1]
    g, r, c = [], [], []

    def row(t, v, cols):
        g.extend([t] * len(cols)), r.extend([v] * len(cols)), c.extend(int(x) for x in cols)

    for t in range(T):                                             # any row, any column: rows that do not exist and columns that
        k = 150                                                    # are no node included; repeats are multi-edges
        rows = rng.integers(0, M, k)
        keep = ~(((t in (0, 4)) & np.isin(rows, (3, 5, 7))) | ((t == 5) & (rows < 2)))
        g.extend([t] * int(keep.sum())), r.extend(rows[keep].tolist()), c.extend(rng.integers(0, M, k)[keep].tolist())
    zero, one = int(np.flatnonzero(colours[0] == 0)[0]), int(np.flatnonzero(colours[0] == 1)[0])
    head = rng.integers(0, M, 256)
    row(0, 3, list(head) + [zero] * 24)                            # 280 entries, equal in the first 256 ...
    row(4, 7, list(head) + [zero] * 23 + [one])                    # ... and different in the last
    same = rng.integers(0, M, 9)
    row(0, 5, same), row(4, 5, same)                               # one class across two graphs
    row(5, 0, [3, 2, 25]), row(5, 1, [3, 2])                       # column 25 is no node of graph 5 (20 nodes): colour -1
    entries = tuple(np.array(a, np.int64) for a in (g, r, c))
    sorted_nbr, classes = ref_sorted_nbr(entries, num_nodes, colours)
    for a in (num_nodes, colours, sorted_nbr, classes) + entries:
        a.setflags(write=False)
    return WlDirect(T, M, num_nodes, colours, entries, sorted_nbr, classes, ((0, 3), (4, 7)), ((5, 0), (5, 1)))


# ---- sp_features -----------------------------------------------------------------------------------------------------------------
SpCase = namedtuple("SpCase", "name T M num_nodes labels num_labels entries directed runs")
SP_FULL_M = (1, 2, 3, 16, 17)
SP_NAMES = ["m128"] + ["full_%d" % m for m in SP_FULL_M] + ["ranks4096", "directed"]
SP_M128_NODES = (0, 1, 2, 3, 16, 17, 23, 64, 90, 91, 127, 128)


def _path(n, start=0):
    return [(start + i + 1, start + i) for i in range(n - 1)]


def _complete(n):
    return [(i, j) for i in range(n) for j in range(i)]


def _m128_pairs(n, rng):
    """what graph the batch at M = 128 holds at n nodes"""
    if n < 2:
        return []
    if n in (2, 128):
        return _path(n)                                            # distances up to 127
    if n in (3, 64, 127):
        return O.cycle(n)
    if n == 16:
        return _complete(16)
    if n == 17:
        return [(i, 0) for i in range(1, 17)]                      # a star
    if n == 23:
        return _path(10) + O.cycle(13, 10)                         # two components
    if n == 90:
        return _path(40)                                           # 50 isolated nodes
    assert n == 91
    tree = [(i, int(rng.integers(0, i))) for i in range(1, 91)]
    return tree + tree + tree                                      # every edge three times


def _stored(graph_pairs):
    """per graph a list of undirected pairs -> (graph, row, col) with every pair stored both ways"""
    g, r, c = [], [], []
    for t, pairs in enumerate(graph_pairs):
        e = O.both_ways(pairs).reshape(-1, 2)
        g.append(np.full(len(e), t, np.int64)), r.append(e[:, 0]), c.append(e[:, 1])
    return tuple(np.concatenate(a + [np.zeros(0, np.int64)]).astype(np.int64) for a in (g, r, c))


def _sp_case(name, M, num_nodes, labels, num_labels, entries, directed):
    num_nodes = np.asarray(num_nodes, np.int32)
    full = np.full((len(num_nodes), M), -1, np.int32)
    for t, lab in enumerate(labels):
        full[t, :num_nodes[t]] = lab
    runs = ref_sp_runs(entries, num_nodes, full, directed)
    for a in (num_nodes, full) + tuple(entries) + runs:
        a.setflags(write=False)
    return SpCase(name, len(num_nodes), M, num_nodes, full, num_labels, entries, directed, runs)


@functools.lru_cache(maxsize=None)
def sp_case(name):
    rng = _rng("sp_" + name)
    if name == "m128":
        nn = SP_M128_NODES
        return _sp_case(name, 128, nn, [rng.integers(0, 3, n) for n in nn], 3, _stored([_m128_pairs(n, rng) for n in nn]), False)
    if name.startswith("full_"):
        M = int(name[5:])
        shapes = [_path(M), _complete(M), O.cycle(M) if M >= 3 else [], [(int(a), int(b)) for a, b in rng.integers(0, M, (2 * M, 2))
                                                                          if a > b]]
        return _sp_case(name, M, [M] * 4, [rng.integers(0, 3, M) for _ in shapes], 3, _stored(shapes), False)
    if name == "ranks4096":
        shapes = [_path(128)] * 32 + [_path(50) + _path(50, 50)]  # the 33rd: 100 nodes, all of rank 4,095, in two components:
        labels = [128 * t + rng.permutation(128) for t in range(32)] + [np.full(100, 4095)]   # 5,000 real keys 0xffffffff
        return _sp_case(name, 128, [128] * 32 + [100], labels, 4096, _stored(shapes), False)  # beside 6,384 padding keys
    assert name == "directed"
    M, nn = 24, (24, 17, 9, 0, 24, 24)
    g, r, c = [], [], []
    for t, n in enumerate(nn[:5]):
        k = 2 * n
        if n:
            g.extend([t] * k), r.extend(rng.integers(0, n, k).tolist()), c.extend(rng.integers(0, M, k).tolist())
    g.extend([5] * 23), r.extend(range(23)), c.extend(range(1, 24))                       # a one-way path: 23 steps forth, none back
    return _sp_case(name, M, nn, [rng.integers(0, 3, n) for n in nn], 3, tuple(np.array(a, np.int64) for a in (g, r, c)), True)


def build_all():
    """every reference of this file once (the lru_caches keep them) -> how many cases"""
    cases = [gram_case(n) for n in GRAM_NAMES] + [wl_runs_case(m) for m in WL_RUNS_M] + [sp_case(n) for n in SP_NAMES]
    cases += [wl_set(), wl_direct()]
    return len(cases)
