#!/usr/bin/env python
"""Generate tests/golden/g13_graph_kernel.npz by RUNNING the reference's own weisfeiler_lehman_subtree_kernel and
shortest_path_kernel in place (graph_kernel/graphkernel/*.py of the reference tree, never copied) over two stand-in modules
written here: `graph_tool.all` (a Graph with vertices(), num_vertices(), vp.nl, out_degree(), and adjacency()) and
`auxiliarymethods.log_primes_list` (logs of the first primes), which the reference imports and does not ship.

Two graph sets, arrays only:
  small_*  41 graphs of <= 13 nodes: a 0-node graph, a 1-node graph, random graphs (p = 0.3, 3 labels; one with a repeated
           entry), and with one label: C6, 2 x C3, the 13-star, an edgeless 5-graph.  Raw and normalised WL (3 iterations, node
           labels and degree labels) and SP Grams.
  two_*    120 graphs of <= 20 nodes in two classes (ring-rich against tree-like), the default data of
           examples/graph_kernel.py: WL and SP Grams and the class labels.
The stand-in adjacency() drops self-loops (the module's stated deviation; these sets hold none).  The generator asserts that
tests/graph_kernel_oracle.py (exact multiset colours) gives the same Grams as the reference (log-prime colours rounded to 10
decimals) on these inputs.

    python tests/golden/make_golden_graph_kernel.py [REFERENCE_ROOT]
"""
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import graph_kernel_oracle as O  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"


# ---- the stand-ins ---------------------------------------------------------------------------------------------------------
class _Vertex:
    def __init__(self, g, i):
        self.g, self.i = g, i

    def out_degree(self):
        return int(self.g.deg[self.i])

    def __index__(self):
        return self.i


class _Props:
    pass


class Graph:
    def __init__(self, n, edges, labels):
        self.n, self.adj = n, O.adjacency(n, edges)
        self.deg = np.asarray(self.adj.sum(axis=1)).reshape(-1).astype(np.int64)
        self.vp = _Props()
        self.vp.nl = {}
        self._v = [_Vertex(self, i) for i in range(n)]
        for v in self._v:
            self.vp.nl[v] = int(labels[v.i])

    def vertices(self):
        return iter(self._v)

    def num_vertices(self):
        return self.n


def _first_primes(count):
    sieve = np.ones(max(16, int(count * (np.log(max(count, 2)) + np.log(np.log(max(count, 3))) + 2))), bool)
    sieve[:2] = False
    for i in range(2, int(len(sieve) ** 0.5) + 1):
        if sieve[i]:
            sieve[i * i::i] = False
    p = np.nonzero(sieve)[0]
    assert len(p) >= count
    return p[:count]


def install_stand_ins(max_vertices):
    gt = types.ModuleType("graph_tool")
    gta = types.ModuleType("graph_tool.all")
    gta.Graph = Graph
    gta.adjacency = lambda g: g.adj
    gt.all = gta
    sys.modules["graph_tool"], sys.modules["graph_tool.all"] = gt, gta
    sys.path.insert(0, os.path.join(REF, "graph_kernel"))
    import auxiliarymethods
    lp = types.ModuleType("auxiliarymethods.log_primes_list")
    lp.log_primes = np.log(_first_primes(max_vertices).astype(np.float64))
    sys.modules["auxiliarymethods.log_primes_list"] = lp
    auxiliarymethods.log_primes_list = lp


# ---- the graph sets --------------------------------------------------------------------------------------------------------
def random_graph(rng, n, p=0.3, num_labels=3):
    pairs = [(i, j) for i in range(n) for j in range(i) if rng.random() < p]
    return n, O.both_ways(pairs), rng.integers(0, num_labels, n)


def small_set():
    rng = np.random.default_rng(13)
    graphs = [(0, np.zeros((0, 2), np.int64), np.zeros(0, np.int64)), (1, np.zeros((0, 2), np.int64), np.array([1]))]
    graphs += [random_graph(rng, int(rng.integers(2, 14))) for _ in range(35)]
    n, e, lab = graphs[5]
    lower = e[e[:, 0] > e[:, 1]]
    assert len(lower)
    graphs[5] = (n, np.concatenate([e, lower[:1]]), lab)             # a repeated entry: a multi-edge
    one = lambda n: np.zeros(n, np.int64)  # noqa: E731
    graphs.append((6, O.both_ways(O.cycle(6)), one(6)))
    graphs.append((6, O.both_ways(O.cycle(3) + O.cycle(3, 3)), one(6)))
    graphs.append((13, O.both_ways([(i, 0) for i in range(1, 13)]), one(13)))
    graphs.append((5, np.zeros((0, 2), np.int64), one(5)))
    assert len(graphs) == 41 and max(g[0] for g in graphs) == 13
    return graphs


def two_class_set():
    rng = np.random.default_rng(120)
    graphs, y = [], []
    for k in range(120):
        n = int(rng.integers(8, 21))
        if k % 2:                                                    # ring-rich: a cycle through all nodes and a few chords
            pairs = set(O.cycle(n))
            for _ in range(int(rng.integers(1, 4))):
                a, b = sorted(rng.choice(n, 2, replace=False))
                pairs.add((int(b), int(a)))
            pairs = sorted({(max(a, b), min(a, b)) for a, b in pairs})
        else:                                                        # tree-like: a random recursive tree
            pairs = [(i, int(rng.integers(0, i))) for i in range(1, n)]
        graphs.append((n, O.both_ways(pairs), rng.integers(0, 3, n)))
        y.append(k % 2)
    return graphs, np.array(y, np.int64)


def reference_grams(graphs, degree=True):
    from graphkernel import shortest_path_kernel_explicit as sp
    from graphkernel import wl_kernel as wl
    db = [Graph(*g) for g in graphs]
    out = {}
    for name, use in (("node", 1), ("degree", 2)) if degree else (("node", 1),):
        out["wl_" + name] = wl.weisfeiler_lehman_subtree_kernel(db, [], 3, True, False, use)
        out["wl_" + name + "_norm"] = wl.weisfeiler_lehman_subtree_kernel(db, [], 3, True, True, use)
        out["sp_" + name] = sp.shortest_path_kernel(db, [], True, False, use)
        out["sp_" + name + "_norm"] = sp.shortest_path_kernel(db, [], True, True, use)
    return out


def main():
    warnings.simplefilter("ignore", DeprecationWarning)
    small, (two, y) = small_set(), two_class_set()
    install_stand_ins(sum(g[0] for g in two) + sum(g[0] for g in small))
    z = {}
    for prefix, graphs in (("small_", small), ("two_", two)):
        z.update(O.pack_graphs(graphs, prefix))
        for key, K in reference_grams(graphs).items():
            kind, lab = key.split("_")[0], key.split("_")[1]
            mine = (O.wl_gram(graphs, 3, lab) if kind == "wl" else O.sp_gram(graphs, lab))
            if key.endswith("_norm"):
                assert np.array_equal(O.normalize(mine), K), key
                z[prefix + key] = np.asarray(K, np.float64)
            else:
                assert np.array_equal(mine.astype(np.float64), K), key      # exact multiset colours == rounded log-primes here
                z[prefix + key] = mine
        print(prefix, "graphs", len(graphs), "max K_ii wl", int(z[prefix + "wl_node"].max()), "sp", int(z[prefix + "sp_node"].max()))
    z["two_y"] = y
    out = os.path.join(HERE, "g13_graph_kernel.npz")
    np.savez_compressed(out, **z)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
