"""The classical graph kernels on the GPU (csrc/graphkern.hip through kgcn_amd/ops.py and kgcn_amd/graph_kernel.py) against the
numpy oracle (tests/graph_kernel_oracle.py) and the fixture the reference produced (tests/golden/g13_graph_kernel.npz).  Every
comparison is exact: colours as partitions, Grams as integers, normalised Grams bit for bit."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import graph_kernel_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "g13_graph_kernel.npz")


@functools.lru_cache(maxsize=None)
def fixture():
    return np.load(GOLDEN, allow_pickle=False)


@functools.lru_cache(maxsize=None)
def small_set():
    return tuple(O.unpack_graphs(fixture(), "small_"))


@functools.lru_cache(maxsize=None)
def cycled(G):
    s = small_set()
    return tuple(s[i % len(s)] for i in range(G))


@functools.lru_cache(maxsize=None)
def oracle_gram(kind, G, labels="node"):
    graphs = list(cycled(G))
    return O.wl_gram(graphs, 3, labels) if kind == "wl" else O.sp_gram(graphs, labels)


def kernel(kind):
    from kgcn_amd import graph_kernel as gk
    return gk.wl_subtree_kernel if kind == "wl" else gk.shortest_path_kernel


def run(kind, graphs, M=None, **kw):
    adjs, nn, lab = O.to_adjs(list(graphs), M)
    return kernel(kind)(adjs, nn, lab, **kw).cpu().numpy()


def same_integers(got, ref):
    assert got.dtype == np.float64 and got.shape == ref.shape
    np.testing.assert_array_equal(got, ref.astype(np.float64))


def runs_and_stats(kind, graphs, chunk_cols=None, M=None):
    """The public route taken apart: the feature runs and gram_from_runs with its column statistics."""
    import torch
    from kgcn_amd import graph_kernel as gk, ops
    adjs, nn, lab = O.to_adjs(list(graphs), M)
    if kind == "wl":
        cols, gs = gk.wl_colourings(adjs, nn, lab, 3)
        runs = [ops.wl_runs(c.reshape(-1), gs.num_nodes, gs.T, gs.M, it << 32) for it, c in enumerate(cols)]
    else:
        gs = gk.GraphSet(adjs, nn, lab)
        col, count = gs.initial_colours("node")
        runs = [ops.sp_features(gs.csr, gs.num_nodes, col, count)]
    col, graph, count = (torch.cat([r[i] for r in runs]) for i in range(3))
    K, stats = ops.gram_from_runs(col, graph, count, gs.T, chunk_cols=chunk_cols, return_stats=True)
    return K.cpu().numpy(), stats, (col.cpu().numpy(), graph.cpu().numpy(), count.cpu().numpy())


# ---- 1. colours after every iteration --------------------------------------------------------------------------------------
@pytest.mark.parametrize("labels", ["node", "degree"])
def test_wl_colours_are_the_oracle_partition_after_every_iteration(labels):
    from kgcn_amd import graph_kernel as gk
    graphs = list(small_set())
    assert len(graphs) == 41
    adjs, nn, lab = O.to_adjs(graphs, 13)
    cols, gs = gk.wl_colourings(adjs, nn, lab, 3, labels)
    ref = O.wl_colours(graphs, 3, labels)
    assert len(cols) == len(ref) == 4 and (gs.T, gs.M) == (41, 13)
    exists = np.arange(13)[None, :] < nn[:, None]
    for it, (c, r) in enumerate(zip(cols, ref)):
        c = c.cpu().numpy()
        assert c.dtype == np.int32 and c.shape == (41, 13)
        assert np.all(c[~exists] == -1) and np.all(c[exists] >= 0), it
        mine = c[exists]                                              # row-major: the oracle's concatenation order
        np.testing.assert_array_equal(O.first_occurrence(mine), O.first_occurrence(r), err_msg="iteration %d" % it)
        assert sorted(set(mine.tolist())) == list(range(len(set(r.tolist())))), it       # dense ids


# ---- 2. forced hash collisions ---------------------------------------------------------------------------------------------
def test_forced_hash_collisions_are_counted_and_refused():
    from kgcn_amd import _lib, graph_kernel as gk, ops
    adjs, nn, lab = O.to_adjs(list(small_set()), 13)
    cols, gs = gk.wl_colourings(adjs, nn, lab, 2)
    col = cols[2].reshape(-1).contiguous()                            # 195 distinct signatures come next, for 256 masked keys:
    #                                                                   about 195^2 / 512 = 74 colliding pairs are expected
    counts = {}
    for mask in (0xF, ops.HASH_MASK_FULL):
        sorted_nbr, hi, lo = ops.wl_refine(gs.csr, gs.num_nodes, col, mask)
        new, info = ops.wl_rank(gs.csr, gs.num_nodes, col, sorted_nbr, hi, lo)
        counts[mask] = info.cpu().numpy().tolist()
        if mask == 0xF:
            keys = hi.cpu().numpy()[:41 * 13][(np.arange(13)[None, :] < nn[:, None]).reshape(-1)]
            assert keys.min() >= 0 and keys.max() <= 0xF
    distinct = len(set(O.wl_colours(list(small_set()), 3)[3].tolist()))
    assert distinct == 195
    assert counts[0xF][1] > 0 and counts[0xF][0] <= 256
    assert counts[ops.HASH_MASK_FULL] == [distinct, 0]
    with pytest.raises(_lib.KgcnHipError, match="differ in their signatures"):
        gk.wl_subtree_kernel(adjs, nn, lab, hash_mask=0xF)
    gk.wl_subtree_kernel(adjs, nn, lab)                               # the full mask passes


# ---- 3. Gram tile and chunk edges ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk_cols", [16, None])
@pytest.mark.parametrize("G", [1, 16, 17, 33, 100])
@pytest.mark.parametrize("kind", ["wl", "sp"])
def test_gram_at_tile_and_chunk_edges(kind, G, chunk_cols):
    got = run(kind, cycled(G), M=13, normalize=False, chunk_cols=chunk_cols)
    same_integers(got, oracle_gram(kind, G))


def labelled_paths(count):
    """Paths of 2 .. count + 1 nodes, graph g with the one label g: no two graphs share a feature."""
    return [(g + 2, O.both_ways([(i + 1, i) for i in range(g + 1)]), np.full(g + 2, 7 * g - 3, np.int64)) for g in range(count)]


@pytest.mark.parametrize("chunk_cols", [16, None])
@pytest.mark.parametrize("kind", ["wl", "sp"])
def test_gram_of_graphs_without_common_features_is_all_diagonal(kind, chunk_cols):
    graphs = labelled_paths(20)
    K, stats, _ = runs_and_stats(kind, graphs, chunk_cols)
    assert stats["dense_columns"] == 0 and stats["diag_columns"] == stats["columns"] > 20
    ref = O.wl_gram(graphs, 3) if kind == "wl" else O.sp_gram(graphs)
    assert not (ref - np.diag(np.diag(ref))).any()
    same_integers(K, ref)


@pytest.mark.parametrize("chunk_cols", [16, None])
@pytest.mark.parametrize("kind", ["wl", "sp"])
def test_gram_of_identical_graphs_is_all_dense(kind, chunk_cols):
    graphs = [small_set()[2]] * 21                                  # 12 nodes
    K, stats, _ = runs_and_stats(kind, graphs, chunk_cols)
    assert stats["diag_columns"] == 0 and stats["dense_columns"] == stats["columns"] > 4
    ref = O.wl_gram(graphs, 3) if kind == "wl" else O.sp_gram(graphs)
    assert len(set(ref.reshape(-1).tolist())) == 1
    same_integers(K, ref)


# ---- 4. exactness above 2^24 -----------------------------------------------------------------------------------------------
def complete(n, start=0):
    return [(start + i, start + j) for i in range(n) for j in range(i)]


@functools.lru_cache(maxsize=None)
def big_set():
    one = lambda n: np.zeros(n, np.int64)  # noqa: E731
    return ((80, O.both_ways(complete(80)), one(80)),
            (80, O.both_ways(complete(80)), np.arange(80) % 2),
            (128, O.both_ways([(i + 1, i) for i in range(127)]), one(128)),
            (80, O.both_ways(complete(40) + complete(40, 40)), one(80)),
            (128, O.both_ways([(i, 0) for i in range(1, 128)]), one(128)))


def test_sp_gram_is_exact_above_2_to_24():
    ref = O.sp_gram(list(big_set()))
    assert 39948800 in np.diag(ref).tolist() and ref.max() > 2 ** 24
    for chunk_cols in (16, None):
        same_integers(run("sp", big_set(), M=128, normalize=False, chunk_cols=chunk_cols), ref)


# ---- 5. limits -------------------------------------------------------------------------------------------------------------
def test_sp_refuses_what_its_key_cannot_hold():
    from kgcn_amd import _lib
    path = (129, O.both_ways([(i + 1, i) for i in range(128)]), np.zeros(129, np.int64))
    with pytest.raises(_lib.KgcnHipError, match="129 nodes a graph, up to 128.*one byte"):
        run("sp", [path])
    many = [(128, np.zeros((0, 2), np.int64), 128 * g + np.arange(128)) for g in range(33)]
    many[32] = (1, np.zeros((0, 2), np.int64), np.array([4096]))      # 32 * 128 + 1 = 4,097 distinct labels
    with pytest.raises(_lib.KgcnHipError, match="4097 distinct labels, up to 4096.*12 \\+ 12 \\+ 8 bits"):
        run("sp", many)
    run("sp", many[:32], normalize=False)                             # 4,096 labels and 128 nodes are served


# ---- 6. invariances --------------------------------------------------------------------------------------------------------
def permuted_nodes(graph, rng):
    n, e, lab = graph
    perm = rng.permutation(n)
    low = O.undirected_edges(n, e)
    pe = perm[low] if len(low) else low
    new = np.zeros(n, np.int64)
    new[perm] = np.asarray(lab)[:n]
    return n, O.both_ways(np.stack([pe.max(axis=1), pe.min(axis=1)], 1)) if len(low) else low, new


@pytest.mark.parametrize("kind", ["wl", "sp"])
def test_invariances(kind):
    graphs = list(small_set())
    base = run(kind, graphs, M=13, normalize=False)
    again = run(kind, graphs, M=13, normalize=False)
    np.testing.assert_array_equal(base.view(np.uint64), again.view(np.uint64))
    rng = np.random.default_rng(5)
    order = rng.permutation(len(graphs))
    np.testing.assert_array_equal(run(kind, [graphs[i] for i in order], M=13, normalize=False), base[np.ix_(order, order)])
    np.testing.assert_array_equal(run(kind, [permuted_nodes(g, rng) for g in graphs], M=13, normalize=False), base)
    np.testing.assert_array_equal(run(kind, graphs, M=16, normalize=False), base)          # more padding rows change nothing


# ---- 7. normalisation ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("labels", ["node", "degree"])
@pytest.mark.parametrize("kind", ["wl", "sp"])
def test_normalised_gram_equals_the_oracle_bit_for_bit(kind, labels):
    graphs = list(small_set())
    got = run(kind, graphs, M=13, normalize=True, labels=labels)
    ref = O.normalize(O.wl_gram(graphs, 3, labels) if kind == "wl" else O.sp_gram(graphs, labels))
    np.testing.assert_array_equal(got.view(np.uint64), ref.view(np.uint64))
    g0 = [g[0] for g in graphs].index(0)
    assert not got[g0].any() and not got[:, g0].any()
    np.testing.assert_array_equal(got.view(np.uint64), fixture()["small_%s_%s_norm" % (kind, labels)].view(np.uint64))


# ---- 8. end to end ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["wl", "sp"])
def test_two_class_fixture_through_the_public_functions(kind):
    from kgcn_amd import graph_kernel as gk
    z = fixture()
    graphs = O.unpack_graphs(z, "two_")
    adjs, nn, lab = O.to_adjs(graphs)
    gs = gk.GraphSet(adjs, nn, lab)                                   # built once, used by both calls
    raw = kernel(kind)(gs, normalize=False).cpu().numpy()
    same_integers(raw, z["two_%s_node" % kind])
    norm = kernel(kind)(gs).cpu().numpy()
    np.testing.assert_array_equal(norm.view(np.uint64), z["two_%s_node_norm" % kind].view(np.uint64))
    feats = kernel(kind)(gs, return_gram=False)
    assert feats.shape[0] == 120 and feats.dtype == np.int64
    np.testing.assert_array_equal(np.asarray((feats @ feats.T).todense()), z["two_%s_node" % kind])
