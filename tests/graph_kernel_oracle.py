"""numpy / scipy oracle of the classical graph kernels (kgcn_amd/graph_kernel.py, csrc/graphkern.hip): the Weisfeiler-Lehman subtree
kernel by explicit (colour, sorted neighbour tuple) signatures, the shortest-path kernel by scipy.sparse.csgraph.shortest_path, and
integer Gram matrices.  Test infrastructure only; it shares no code with the module under test.

A graph is (n, edges [E, 2], labels [n]): edges as a dataset stores them (either or both directions, self-loops, repeats).  As
graph_kernel/dataset2graph.py:56-57 does, only entries with row >= col are read, each as one undirected edge occurrence (a repeat is
a multi-edge); self-loops are dropped (the module's stated deviation)."""
import numpy as np
import scipy.sparse as sps
import scipy.sparse.csgraph as csg


def undirected_edges(n, edges):
    """-> [E', 2] (row > col) edge occurrences of the graph."""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    e = e[e[:, 0] > e[:, 1]]
    assert e.size == 0 or (e.min() >= 0 and e.max() < n)
    return e


def neighbours(n, edges):
    """-> per node the list of its neighbours, one item per edge occurrence."""
    nb = [[] for _ in range(n)]
    for r, c in undirected_edges(n, edges):
        nb[r].append(int(c))
        nb[c].append(int(r))
    return nb


def adjacency(n, edges):
    """-> scipy CSR [n, n] of edge multiplicities (what a graph library's adjacency() of the undirected multigraph gives)."""
    e = undirected_edges(n, edges)
    a = sps.coo_matrix((np.ones(2 * len(e)), (np.r_[e[:, 0], e[:, 1]], np.r_[e[:, 1], e[:, 0]])), shape=(n, n))
    return a.tocsr()


def dense_ranks(values):
    """np.unique(..., return_inverse=True)[1] of the concatenated values."""
    values = np.asarray(values)
    return np.unique(values, return_inverse=True)[1].reshape(-1).astype(np.int64) if values.size else np.zeros(0, np.int64)


def initial_colours(graphs, labels="node"):
    """Dense ranks over the whole set of the node labels, or of the degrees (labels="degree": the reference's use_labels == 2)."""
    if labels == "node":
        raw = [np.asarray(lab, np.int64)[:n] for n, _, lab in graphs]
    elif labels == "degree":
        raw = [np.array([len(x) for x in neighbours(n, e)], np.int64) for n, e, _ in graphs]
    else:
        raise ValueError(labels)
    return dense_ranks(np.concatenate(raw) if raw else np.zeros(0, np.int64))


def wl_colours(graphs, iterations, labels="node"):
    """-> [iterations + 1] colour vectors over the concatenated nodes of the set: colours[0] the initial ones, colours[i + 1] the
    ids (in order of first occurrence) of the classes of (colours[i][v], sorted colours[i] of v's neighbours)."""
    offs = np.concatenate([[0], np.cumsum([g[0] for g in graphs])]).astype(np.int64)
    nbs = [neighbours(n, e) for n, e, _ in graphs]
    col = initial_colours(graphs, labels)
    out = [col]
    for _ in range(iterations):
        ids, new = {}, np.zeros_like(col)
        for g, nb in enumerate(nbs):
            for v, lst in enumerate(nb):
                sig = (int(col[offs[g] + v]), tuple(sorted(int(col[offs[g] + u]) for u in lst)))
                new[offs[g] + v] = ids.setdefault(sig, len(ids))
        col = new
        out.append(col)
    return out


def first_occurrence(ids):
    """Relabel ids in the order of their first occurrence: two labelings are one partition iff this gives equal arrays."""
    seen, out = {}, np.zeros(len(ids), np.int64)
    for i, v in enumerate(ids):
        out[i] = seen.setdefault(int(v), len(seen))
    return out


def _csr_from_keys(per_graph_keys):
    """per graph a list of hashable feature keys (one per occurrence) -> integer scipy CSR [G, F] of counts."""
    ids, rows, cols = {}, [], []
    for g, keys in enumerate(per_graph_keys):
        for k in keys:
            rows.append(g)
            cols.append(ids.setdefault(k, len(ids)))
    m = sps.coo_matrix((np.ones(len(rows), np.int64), (rows, cols)), shape=(len(per_graph_keys), max(len(ids), 1)))
    return m.tocsr()


def wl_features(graphs, iterations=3, labels="node"):
    offs = np.concatenate([[0], np.cumsum([g[0] for g in graphs])]).astype(np.int64)
    cols = wl_colours(graphs, iterations, labels)
    return _csr_from_keys([[(it, int(c)) for it, col in enumerate(cols) for c in col[offs[g]:offs[g + 1]]]
                           for g in range(len(graphs))])


def sp_distances(n, edges):
    """[n, n] float distances, inf for unreachable pairs."""
    if n == 0:
        return np.zeros((0, 0))
    return csg.shortest_path(adjacency(n, edges), method="D", directed=False, unweighted=True)


def sp_features(graphs, labels="node"):
    offs = np.concatenate([[0], np.cumsum([g[0] for g in graphs])]).astype(np.int64)
    col = initial_colours(graphs, labels)
    per = []
    for g, (n, e, _) in enumerate(graphs):
        d, lab = sp_distances(n, e), col[offs[g]:offs[g + 1]]
        per.append([(int(lab[k]), int(lab[j]), float(d[k, j])) for k in range(n) for j in range(n)])
    return _csr_from_keys(per)


def gram(features):
    """Integer Gram [G, G] of an integer count matrix."""
    f = features.astype(np.int64)
    return np.asarray((f @ f.T).todense(), np.int64)


def wl_gram(graphs, iterations=3, labels="node"):
    return gram(wl_features(graphs, iterations, labels))


def sp_gram(graphs, labels="node"):
    return gram(sp_features(graphs, labels))


def normalize(K):
    """auxiliary_methods.normalize_gram_matrix: K_ij / sqrt(K_ii K_jj), 0 where either diagonal entry is 0 (float64)."""
    K = np.asarray(K, np.float64)
    d = np.diag(K)
    prod = d[:, None] * d[None, :]
    ok = (d[:, None] != 0.0) & (d[None, :] != 0.0)
    return np.where(ok, K / np.sqrt(np.where(ok, prod, 1.0)), 0.0)


# ---- the graph sets of the fixture and the GPU tests ---------------------------------------------------------------------------
def cycle(n, start=0):
    """Undirected pairs of the n-cycle on nodes start .. start + n - 1."""
    return [(start + (i + 1) % n, start + i) for i in range(n)]


def both_ways(pairs):
    """Undirected pairs -> entries in both directions (how kGCN datasets store an adjacency)."""
    p = np.asarray(pairs, np.int64).reshape(-1, 2)
    return np.concatenate([p, p[:, ::-1]]) if len(p) else p


def unpack_graphs(z, prefix):
    """Fixture arrays -> [(n, edges, labels)]."""
    nn, eo, e, lab = z[prefix + "num_nodes"], z[prefix + "edge_offsets"], z[prefix + "edges"], z[prefix + "labels"]
    lo = np.concatenate([[0], np.cumsum(nn)])
    return [(int(nn[g]), e[eo[g]:eo[g + 1]], lab[lo[g]:lo[g + 1]]) for g in range(len(nn))]


def pack_graphs(graphs, prefix):
    return {prefix + "num_nodes": np.array([g[0] for g in graphs], np.int32),
            prefix + "edge_offsets": np.concatenate([[0], np.cumsum([len(g[1]) for g in graphs])]).astype(np.int64),
            prefix + "edges": (np.concatenate([np.asarray(g[1], np.int32).reshape(-1, 2) for g in graphs])
                               if graphs else np.zeros((0, 2), np.int32)),
            prefix + "labels": np.concatenate([np.asarray(g[2], np.int32) for g in graphs]) if graphs else np.zeros(0, np.int32)}


def to_adjs(graphs, M=None):
    """-> (adjs[b][0] = (idx [E, 2], val [E], (M, M)), num_nodes [T], node_labels [T, M]) for the public functions."""
    M = max([g[0] for g in graphs] + [1]) if M is None else M
    adjs, lab = [], np.zeros((len(graphs), M), np.int64)
    for g, (n, e, l) in enumerate(graphs):
        e = np.asarray(e, np.int64).reshape(-1, 2)
        adjs.append([(e, np.ones(len(e), np.float32), (M, M))])
        lab[g, :n] = np.asarray(l)[:n]
    return adjs, np.array([g[0] for g in graphs], np.int32), lab
