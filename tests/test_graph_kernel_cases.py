"""CPU checks of tests/graph_kernel_cases.py, the cases tests/test_gpu_graph_kernel_ops.py runs on the device: its plain references
give the oracle's Grams on the fixture's small set (tests/graph_kernel_oracle.py shares no code with them), and every case has the
property it is named for -- the tile rows and the dense column count against chunk_cols, the bit pairs, the empty tile row, entries
of K between 2^32 and 2^53, runs longer than a thread's segment, a degree above 256, n^2 against its power of two, label rank 4,095
at a real distance and at 255, a CSR that is not symmetric.  A case that loses its property fails here and never as a GPU pass
that means nothing.  The time all references take together is printed (pytest -s / -rP); the docstring of graph_kernel_cases.py
carries the figure."""
import os
import time

import numpy as np
import pytest

import graph_kernel_cases as C
import graph_kernel_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g13_graph_kernel.npz")


def small_set():
    return O.unpack_graphs(np.load(GOLDEN, allow_pickle=False), "small_")


def padded(graphs, vector, M, fill=-1):
    """a vector over the concatenated nodes -> [T, M]"""
    out, at = np.full((len(graphs), M), fill, np.int64), 0
    for t, (n, _, _) in enumerate(graphs):
        out[t, :n] = vector[at:at + n]
        at += n
    return out


def direct_stats(features):
    occ = np.asarray((features > 0).sum(0)).reshape(-1)
    return int((occ > 0).sum()), int((occ == 1).sum()), int((occ > 1).sum())


# ---- the references against the oracle ---------------------------------------------------------------------------------------------
def test_references_give_the_oracle_grams_on_the_small_set():
    graphs = small_set()
    nn = np.array([g[0] for g in graphs])
    assert len(graphs) == 41 and nn.max() == 13
    runs = [C.ref_wl_runs(padded(graphs, c, 13), nn, it << 32) for it, c in enumerate(O.wl_colours(graphs, 3))]
    col, graph, count = (np.concatenate([r[i] for r in runs]) for i in (1, 2, 3))
    K, stats = C.ref_gram(col, graph, count, 41)
    np.testing.assert_array_equal(K, O.wl_gram(graphs, 3))
    assert stats == direct_stats(O.wl_features(graphs, 3))
    pairs = [O.undirected_edges(n, e) for n, e, _ in graphs]
    entries = tuple(np.concatenate([np.full(len(p), t) if k < 0 else p[:, k] for t, p in enumerate(pairs)]) for k in (-1, 0, 1))
    ptr, col, graph, count = C.ref_sp_runs(entries, nn, padded(graphs, O.initial_colours(graphs), 13), directed=False)
    K, stats = C.ref_gram(col, graph, count, 41)
    np.testing.assert_array_equal(K, O.sp_gram(graphs))
    assert stats == direct_stats(O.sp_features(graphs))
    assert ptr[0] == 0 and ptr[-1] == len(col) and np.array_equal(np.diff(ptr), np.bincount(graph, minlength=41))


def test_reference_runs_are_in_the_documented_order():
    for runs in [C.wl_runs_case(m).runs for m in C.WL_RUNS_M] + [C.sp_case(n).runs for n in C.SP_NAMES]:
        ptr, col, graph, count = runs
        assert np.all(np.diff(graph) >= 0) and np.all(count > 0)
        for t in range(len(ptr) - 1):
            assert np.all(graph[ptr[t]:ptr[t + 1]] == t)
            assert np.all(np.diff(col[ptr[t]:ptr[t + 1]].view(np.uint64).astype(object)) > 0)


# ---- Gram ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.GRAM_NAMES)
def test_gram_case_is_what_its_name_says(name):
    case = C.gram_case(name)
    G, chunk, dense = case.spec
    assert case.stats[2] == dense and case.stats[0] == case.stats[1] + dense and case.stats[1] >= 9
    tiles = -(-G // C.TILE)
    assert tiles == {1: 1, 64: 1, 65: 2, 128: 2, 129: 3, 193: 4, 260: 5}[G]
    live = sorted(set(case.graph.tolist()))
    assert sorted(set(range(G)) - set(live)) == list(case.empty)
    assert G - 1 in live and (G < 8 or len(case.empty) >= 2)
    if tiles >= 3:                                                  # one tile row of graphs without a run, the others live
        rows = {g // C.TILE for g in live}
        assert len(rows) == tiles - 1
        assert not case.K[[g for g in range(G) if g // C.TILE not in rows]].any()
    if dense and tiles == 5:                                        # every tile distance has a non-zero entry above the diagonal
        far = {(j // C.TILE) - (i // C.TILE) for i, j in zip(*np.nonzero(np.triu(case.K, 1)))}
        assert far == {0, 1, 2, 4} | {3}
    keys = set(case.col.view(np.uint64).tolist())
    for bit in C.BIT_PAIRS:
        assert any(k ^ (1 << bit) in keys for k in keys), bit
    assert case.col.min() < 0                                       # bit 63 makes the int64 negative
    assert np.any(np.diff(case.col.view(np.uint64).astype(object)) < 0) and (G == 1 or np.any(np.diff(case.graph) < 0))  # sorted by neither
    assert len(set(zip(case.col.tolist(), case.graph.tolist()))) == len(case.col)
    assert case.count.min() >= 1 and case.count.max() == 2 ** 20
    assert 2 ** 32 < case.K.max() < 2 ** 53 and np.array_equal(case.K, case.K.T)
    for g in case.empty:
        assert not case.K[g].any()


def test_gram_cases_cover_the_chunk_edges():
    have = {(s.chunk_cols, s.dense) for s in C.GRAM_SPECS.values()}
    assert {(16, d) for d in (0, 1, 15, 16, 17, 33)} <= have
    assert {(None, d) for d in (1023, 1024, 1025)} <= have
    assert any(cc == 16 and d > 48 for cc, d in have) and any(cc is None and d > 2 * C.DEFAULT_CHUNK for cc, d in have)
    assert {(s.G, s.chunk_cols) for s in C.GRAM_SPECS.values()} == {(G, cc) for G in (1, 64, 65, 128, 129, 193, 260) for cc in (16, None)}
    import re
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "kgcn_amd", "ops.py")).read()
    assert int(re.search(r"^GRAM_CHUNK_COLS = (\d+)", src, re.M).group(1)) == C.DEFAULT_CHUNK


# ---- wl_runs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", C.WL_RUNS_M)
def test_wl_runs_case_is_what_its_name_says(M):
    case = C.wl_runs_case(M)
    assert 3 <= case.T <= 5 and case.colours.shape == (case.T, M) and case.colours.dtype == np.int32
    assert set(case.num_nodes.tolist()) <= {0, 1, M - 1, M} and case.num_nodes[0] == M
    ptr, col, graph, count = case.runs
    per = (M + 255) // 256                                          # emit_runs' segment at n = M
    for t, pattern in enumerate(case.patterns):
        n, cnt = int(case.num_nodes[t]), count[ptr[t]:ptr[t + 1]]
        assert cnt.sum() == n
        if pattern == "three" and n >= 3:
            assert len(cnt) == 3 and (n < 30 or cnt.min() > 2 * per)  # a run crosses several segments
        if pattern == "distinct":
            assert len(cnt) == n and (n == 0 or col[ptr[t + 1] - 1] == C.WL_RUNS_OFFSET + C.MAX_COLOUR)
        if pattern == "equal":
            assert len(cnt) == min(n, 1)
        assert np.all(case.colours[t, n:] == C.PAD_JUNK)
    assert case.colours.max() == C.MAX_COLOUR or M == 1
    assert np.all(col >> 32 == 3)
    if M == 4096:
        assert per == 16 and case.num_nodes.tolist() == [4096, 4095, 4096, 1, 0]


# ---- the graph set ---------------------------------------------------------------------------------------------------------------
def test_wl_set_is_what_it_says():
    s = C.wl_set()
    nn = np.array([g[0] for g in s.graphs])
    assert len(s.graphs) == 208 and nn.max() == C.WL_M and len(s.graphs) * C.WL_M > 60000
    assert nn[:200].min() >= 40 and {int(l) for g in s.graphs[:200] for l in g[2]} == {0, 1}
    assert max_entry_run(s.graphs[s.index["star_a"]]) == 299 and C.max_degree(s.graphs[s.index["star_a"]]) >= 257
    a, b = s.graphs[s.index["star_a"]], s.graphs[s.index["star_b"]]
    assert np.array_equal(a[1], b[1]) and np.flatnonzero(a[2] != b[2]).tolist() == [299]
    assert C.max_degree(s.graphs[s.index["k24"]]) == 23
    n, e, _ = s.graphs[s.index["tripled"]]
    low = [tuple(p) for p in O.undirected_edges(n, e).tolist()]
    assert low and all(low.count(p) % 3 == 0 for p in set(low))
    assert (nn[s.index["none"]], nn[s.index["one"]]) == (0, 1)
    offs = np.concatenate([[0], np.cumsum(nn)])
    tri, hexa = s.index["triangles"], s.index["hexagon"]
    for it, c in enumerate(s.colours):                              # what WL cannot tell apart
        assert sorted(c[offs[tri]:offs[tri + 1]].tolist()) == sorted(c[offs[hexa]:offs[hexa + 1]].tolist()), it
        ca, cb = c[offs[s.index["star_a"]]], c[offs[s.index["star_b"]]]
        assert (ca == cb) == (it == 0)                              # the centres part at the first refinement
    assert s.gram[tri, tri] == s.gram[tri, hexa] == s.gram[hexa, hexa]
    assert s.columns[1] > 0 and s.columns[2] > 0 and not s.gram[s.index["none"]].any()
    assert len(set(s.colours[-1].tolist())) > 10000                 # many classes: the ranking is no single-block sort


def max_entry_run(graph):
    """the longest row of the symmetrised storage"""
    n, e, _ = graph
    low = O.undirected_edges(n, e)
    return int(np.bincount(np.r_[low[:, 0], low[:, 1]], minlength=max(n, 1)).max()) if len(low) else 0


def test_wl_direct_is_what_it_says():
    d = C.wl_direct()
    g, r, c = d.entries
    stored = set(zip(g.tolist(), r.tolist(), c.tolist()))
    assert any((t, b, a) not in stored for t, a, b in stored)       # not symmetric
    assert len(stored) < len(g)                                     # repeated entries
    assert np.any(r >= d.num_nodes[g]) and np.any((c >= d.num_nodes[g]) & (r < d.num_nodes[g]))
    (ta, ra), (tb, rb) = d.long_rows
    ea, eb = c[(g == ta) & (r == ra)], c[(g == tb) & (r == rb)]
    assert len(ea) == len(eb) == 280 and d.colours[ta, ra] == d.colours[tb, rb]
    np.testing.assert_array_equal(d.colours[ta][ea[:256]], d.colours[tb][eb[:256]])
    assert d.classes[ta, ra] != d.classes[tb, rb] and d.classes[0, 5] == d.classes[4, 5]
    (t, ra), (_, rb) = d.pad_rows                                   # equal but for one entry whose column is no node
    ea, eb = c[(g == t) & (r == ra)], c[(g == t) & (r == rb)]
    assert d.colours[t, ra] == d.colours[t, rb] and sorted(ea[ea < d.num_nodes[t]]) == sorted(eb) and np.sum(ea >= d.num_nodes[t]) == 1
    assert d.classes[t, ra] != d.classes[t, rb] and -1 in d.sorted_nbr
    exists = np.arange(d.M)[None, :] < d.num_nodes[:, None]
    assert np.all((d.classes >= 0) == exists) and len(d.sorted_nbr) == len(g)
    assert len(set(d.classes[exists].tolist())) < exists.sum()      # classes with several rows, beside the planted pair


# ---- shortest paths --------------------------------------------------------------------------------------------------------------
def np2(x):
    p = 1
    while p < x:
        p <<= 1
    return p


@pytest.mark.parametrize("name", C.SP_NAMES)
def test_sp_case_is_what_its_name_says(name):
    case = C.sp_case(name)
    ptr, col, graph, count = case.runs
    nn = case.num_nodes.astype(np.int64)
    np.testing.assert_array_equal(np.add.reduceat(np.r_[count, 0], ptr[:-1]) * (np.diff(ptr) > 0), nn * nn)      # every ordered pair once
    dist, lk, lj = col & 0xff, (col >> 20) & 0xfff, (col >> 8) & 0xfff
    assert col.min(initial=0) >= 0 and col.max(initial=0) <= 0xffffffff and lk.max(initial=0) < case.num_labels
    g, r, c = case.entries
    stored = set(zip(g.tolist(), r.tolist(), c.tolist()))
    assert case.directed == any((t, b, a) not in stored for t, a, b in stored)
    if name == "m128":
        assert tuple(nn) == C.SP_M128_NODES and case.M == 128
        assert {int(n * n) for n in nn if n and np2(n * n) == n * n} >= {256, 16384}          # nn == np2 exactly
        assert {int(n * n) - np2(n * n) // 2 for n in (17, 23, 91)} == {33, 17, 89}           # just past a power of two
        real = dist[dist < 255]
        assert real.max() == 127 and 255 in dist and len(stored) < len(g)                     # the long path; components; repeats
    if name.startswith("full_"):
        assert np.all(nn == case.M) and case.M == int(name[5:])
    if name == "ranks4096":
        assert case.num_labels == 4096 and len(set(case.labels[:32].reshape(-1).tolist())) == 4096
        assert any(0 < d < 255 for d in dist[(lk == 4095) & (graph == 31)].tolist())          # rank 4,095 at real distances
        last = graph == 32                                          # the key that is also the padding key, 5,000 times, in a graph
        assert count[last & (col == 0xffffffff)].tolist() == [5000] and np2(100 * 100) > 100 * 100      # whose n^2 is padded
        assert np.all(lk[last] == 4095) and np.all(lj[last] == 4095) and dist[last].tolist() == list(range(50)) + [255]
    if name == "directed":
        assert np.any((c >= nn[g]) & (c < case.M))
        way = graph == 5                                           # the one-way path is walked forth and never back
        assert dist[way].max() == 255 and count[way & (dist == 255)].sum() == 23 * 24 // 2 and 23 in dist[way]


def test_all_references_build_in_seconds():
    for f in (C.gram_case, C.wl_runs_case, C.wl_graphs, C.wl_set, C.wl_direct, C.sp_case):
        f.cache_clear()
    t0 = time.perf_counter()
    n = C.build_all()
    took = time.perf_counter() - t0
    print("graph_kernel_cases: the references of %d cases built in %.1f s" % (n, took))
    assert n == len(C.GRAM_NAMES) + len(C.WL_RUNS_M) + len(C.SP_NAMES) + 2 and took < 30
