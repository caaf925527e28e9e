#!/usr/bin/env python
"""Generate tests/golden/g14_hash_kernel.npz by RUNNING the reference's hash graph kernel pieces in place
(graph_kernel/auxiliarymethods/auxiliary_methods.py locally_sensitive_hashing, graphkernel/wl_kernel.py,
graphkernel/shortest_path_kernel_explicit.py of the reference tree, never copied) over the stand-ins of
make_golden_graph_kernel.py plus a `vp.na` attribute property.

hash_graph_kernel.py itself runs only for the shortest-path base kernel and flattened hashes (sparse.hstack of the Weisfeiler-Lehman
kernel's lists of arrays stops with "blocks must be 2-D", np.array([colors_0, colors_1]) stops on unflattened hashes), so the
pieces are called one draw at a time, as its loop at lines 42-57 does, and combined as its lines 57-66 say: hstack, sqrt(1 / R) *
F, F.dot(F.T), normalize_gram_matrix.  locally_sensitive_hashing is wrapped to record what np.random gave it, (v, b) of every
draw, and to flatten its result.

Arrays only:
  small_*      the 41 graphs of g13's small_ set with the 0-node graph moved off the first place, small_attr [272, 5]: attributes
               correlated with the node labels, small_scaled: sklearn.preprocessing.scale of them (hash_graph_kernel.py:40)
  r3_*, r20_*  for R = 3 and R = 20 draws: V [R, 5], b [R], hashes [R, 272] as the reference returned them, min_dist: the
               smallest distance of any (x . v + b) / w to an integer, and for wl_u0 (use_labels 0), wl_u1 (use_labels 1),
               sp_u0: the raw and the normalised Gram and the column count of the stacked feature matrix
  two_attr     attributes for the 120-graph two_ set of g13 (the default data of examples/graph_kernel.py --kernel hgk-*)
The generator asserts min_dist >= 1e-9 (pick another seed if not): the buckets then do not depend on the summation order.

    python tests/golden/make_golden_hash_kernel.py [REFERENCE_ROOT]
"""
import math
import os
import sys
import warnings

import numpy as np
import scipy.sparse as sparse

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import graph_kernel_oracle as O  # noqa: E402
import hash_kernel_oracle as H  # noqa: E402
import make_golden_graph_kernel as G13  # noqa: E402

D, W, SIGMA, WL_ITERATIONS = 5, 1.0, 1.0, 3


class AttrGraph(G13.Graph):
    def __init__(self, n, edges, labels, attrs):
        super().__init__(n, edges, labels)
        self.vp.na = {v: attrs[v.i] for v in self._v}


def attributes(graphs, seed):
    """[Nv, D]: column j = (label - 1) * a_j + noise, so that buckets and labels are correlated but not the same."""
    rng = np.random.default_rng(seed)
    lab = np.concatenate([np.asarray(g[2], np.float64)[:g[0]] for g in graphs])
    slope = rng.uniform(0.5, 2.0, D)
    return (lab[:, None] - 1.0) * slope[None, :] + rng.standard_normal((len(lab), D)) * 0.75 + rng.uniform(-3, 3, D)[None, :]


def recording_lsh(aux, record):
    """aux.locally_sensitive_hashing, flattened, with the numbers np.random gave it appended to record as (v [d], b)."""
    inner = aux.locally_sensitive_hashing

    def wrapped(m, d, w, sigma=1.0):
        randn, rand, got = np.random.randn, np.random.rand, {}

        def randn_spy(*shape):
            got["v"] = randn(*shape)
            return got["v"]

        def rand_spy(*shape):
            got["b"] = rand(*shape)
            return got["b"]
        np.random.randn, np.random.rand = randn_spy, rand_spy
        try:
            out = inner(m, d, w, sigma=sigma)
        finally:
            np.random.randn, np.random.rand = randn, rand
        record.append((np.asarray(got["v"], np.float64).reshape(-1) * sigma, float(w * got["b"] * sigma), m))
        return np.asarray(out).ravel()
    return wrapped


def combine(per_draw, normalize, aux):
    """hash_graph_kernel.py:57-66 over the per-draw feature matrices."""
    feature_vectors = per_draw[0]
    for tmp in per_draw[1:]:
        feature_vectors = sparse.hstack((feature_vectors, tmp))
    feature_vectors = feature_vectors.tocsr()
    columns = feature_vectors.shape[1]
    feature_vectors = math.sqrt(1.0 / len(per_draw)) * feature_vectors
    gram = feature_vectors.dot(feature_vectors.T).toarray()
    return (aux.normalize_gram_matrix(gram) if normalize else gram), columns


def main():
    warnings.simplefilter("ignore", DeprecationWarning)
    if len(sys.argv) > 1:
        G13.REF = sys.argv[1]
    z13 = np.load(os.path.join(HERE, "g13_graph_kernel.npz"), allow_pickle=False)
    small = O.unpack_graphs(z13, "small_")
    zero = [g[0] for g in small].index(0)
    small = small[:zero] + small[zero + 1:8] + [small[zero]] + small[8:]             # the 0-node graph not first
    assert len(small) == 41 and small[0][0] > 0 and small[7][0] == 0
    two = O.unpack_graphs(z13, "two_")
    G13.install_stand_ins(sum(g[0] for g in small) + sum(g[0] for g in two))
    from auxiliarymethods import auxiliary_methods as aux
    from graphkernel import shortest_path_kernel_explicit as sp
    from graphkernel import wl_kernel as wl
    from sklearn import preprocessing as pre

    X = attributes(small, 14)
    assert X.shape == (272, D)
    scaled = pre.scale(X, axis=0)                                                    # hash_graph_kernel.py:40
    offs = np.concatenate([[0], np.cumsum([g[0] for g in small])])
    db = [AttrGraph(n, e, lab, X[offs[g]:offs[g + 1]]) for g, (n, e, lab) in enumerate(small)]
    z = dict(O.pack_graphs(small, "small_"))
    z["small_attr"], z["small_scaled"] = X, scaled
    z["two_attr"] = attributes(two, 120)

    mine_scaled = H.scale_attributes(X)[0]
    assert np.abs(mine_scaled - scaled).max() <= 272 * 2.0 ** -52 * np.abs(scaled).max()
    for R, seed in ((3, 143), (20, 1420)):
        np.random.seed(seed)
        record = []
        lsh = recording_lsh(aux, record)
        hashes = [lsh(scaled, D, W, sigma=SIGMA) for _ in range(R)]                  # hash_graph_kernel.py:43
        V, b = np.stack([r[0] for r in record]), np.array([r[1] for r in record])
        z_ref = np.stack([(np.dot(scaled, V[r][:, None]).ravel() + b[r]) / W for r in range(R)])
        dist = min(float(np.abs(z_ref - np.round(z_ref)).min()), H.boundary_distance(mine_scaled, V, b, W))
        assert dist >= 1e-9, (R, seed, dist)
        mine = H.buckets(mine_scaled, V, b, W)
        for r in range(R):
            assert np.array_equal(O.first_occurrence(mine[r]), O.first_occurrence(hashes[r])), (R, r)
        p = "r%d_" % R
        z[p + "V"], z[p + "b"], z[p + "hashes"], z[p + "min_dist"] = V, b, np.stack(hashes).astype(np.int32), np.float64(dist)
        per = {"wl_u0": [sparse.csr_matrix(np.array(wl.weisfeiler_lehman_subtree_kernel(db, h, WL_ITERATIONS, False, False, 0)))
                         for h in hashes],
               "wl_u1": [sparse.csr_matrix(np.array(wl.weisfeiler_lehman_subtree_kernel(db, h, WL_ITERATIONS, False, False, 1)))
                         for h in hashes],
               "sp_u0": [sparse.csr_matrix(sp.shortest_path_kernel(db, h, False, False, 0)) for h in hashes]}
        for name, feats in per.items():
            raw, cols = combine(feats, False, aux)
            norm, _ = combine(feats, True, aux)
            base, labels = name.split("_")[0], (None if name.endswith("u0") else "node")
            exact = H.exact_gram(H.hash_features(small, mine, base, WL_ITERATIONS, labels))
            bound = (cols + 8) * 2.0 ** -53
            err = float(np.abs(raw - exact).max() / np.abs(exact).max())
            assert err <= bound, (name, R, err, bound)                               # exact multiset colours == log-primes here
            z[p + name], z[p + name + "_norm"], z[p + name + "_columns"] = raw, norm, np.int64(cols)
            print("R", R, name, "columns", cols, "max rel diff of the float path to exact F F^T / R: %.3g (bound %.3g)" % (err, bound),
                  "min distance to a bucket boundary %.3g" % dist)
    out = os.path.join(HERE, "g14_hash_kernel.npz")
    np.savez_compressed(out, **z)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
