"""numpy oracle of the hash graph kernels (kgcn_amd/graph_kernel.py hash_graph_kernel, csrc/hashkern.hip), built on
tests/graph_kernel_oracle.py.  Test infrastructure only; it shares no code with the module under test.

A graph set is [(n, edges, labels)] as in graph_kernel_oracle, its attributes X [Nv, d] float64: the rows of all nodes in graph
order.  What the reference computes (graph_kernel/graphkernel/hash_graph_kernel.py, auxiliarymethods/auxiliary_methods.py:23-36):
scale the columns, draw R projections, bucket every node by floor((x . v + b) / w), run the base kernel on the dense ranks of the
buckets, stack the R feature maps, K = F F^T / R.  The floating-point steps are restated in the order the kernels state, so that
the comparison with the device is bit for bit:
  * column sums: rows added one after another inside chunks of 256 rows, then the chunk sums in ascending order, every sum
    starting from +0.0 (np.cumsum is sequential);
  * the projection: acc = 0, acc = acc + x_k * v_k for k ascending; numpy fuses nothing."""
import numpy as np

import graph_kernel_oracle as O

CHUNK = 256


def chunked_column_sums(a):
    """[rows, d] -> [d]: sequential sums inside chunks of 256 rows, then sequentially over the chunks, from +0.0."""
    a = np.asarray(a, np.float64)
    zero = np.zeros((1, a.shape[1]))
    parts = [np.cumsum(np.concatenate([zero, a[r0:r0 + CHUNK]]), axis=0)[-1] for r0 in range(0, a.shape[0], CHUNK)]
    return np.cumsum(np.concatenate([zero, np.stack(parts)]), axis=0)[-1]


def scale_attributes(X):
    """-> (scaled, mean, std): sklearn.preprocessing.scale in the stated order; a column of equal values becomes 0."""
    X = np.asarray(X, np.float64)
    rows = np.float64(X.shape[0])
    mean = chunked_column_sums(X) / rows
    dv = X - mean
    std = np.sqrt(chunked_column_sums(dv * dv) / rows)
    return dv / np.where(std == 0.0, 1.0, std), mean, std


def projected(X, v, b, w):
    """(x . v + b) / w of every row, the dot product added for k ascending."""
    X = np.asarray(X, np.float64)
    acc = np.zeros(X.shape[0])
    for k in range(X.shape[1]):
        acc = acc + X[:, k] * np.float64(v[k])
    return (acc + np.float64(b)) / np.float64(w)


def buckets(X, V, b, w):
    """[R, Nv] int64: floor((x . v_r + b_r) / w)."""
    return np.stack([np.floor(projected(X, V[r], b[r], w)).astype(np.int64) for r in range(len(V))])


def boundary_distance(X, V, b, w):
    """The smallest distance of any (x . v_r + b_r) / w to an integer."""
    z = np.stack([projected(X, V[r], b[r], w) for r in range(len(V))])
    return float(np.abs(z - np.round(z)).min()) if z.size else 1.0


def with_labels(graphs, per_node):
    """The graphs with per_node (over the concatenated nodes) as their labels."""
    offs = np.concatenate([[0], np.cumsum([g[0] for g in graphs])]).astype(np.int64)
    return [(n, e, np.asarray(per_node[offs[g]:offs[g + 1]], np.int64)) for g, (n, e, _) in enumerate(graphs)]


def _per_graph(graphs, per_node_keys):
    offs = np.concatenate([[0], np.cumsum([g[0] for g in graphs])]).astype(np.int64)
    return [per_node_keys[offs[g]:offs[g + 1]] for g in range(len(graphs))]


def wl_hash_features(graphs, hashed, iterations=3, labels=None):
    """One draw of wl_kernel.py:61-92 -> integer CSR [G, F].  labels None (use_labels == 0): the hashed colours are refined and
    counted.  labels "node" | "degree": label colours and hashed colours are refined separately and every iteration counts the
    joint classes (c0, c1)."""
    hashed = O.dense_ranks(hashed)
    c1 = O.wl_colours(with_labels(graphs, hashed), iterations, "node")
    if labels is None:
        keys = [[(it, int(c)) for c in col] for it, col in enumerate(c1)]
    else:
        c0 = O.wl_colours(graphs, iterations, labels)
        keys = [[(it, int(a), int(c)) for a, c in zip(c0[it], c1[it])] for it in range(iterations + 1)]
    per_it = [_per_graph(graphs, k) for k in keys]
    return O._csr_from_keys([[key for it in range(iterations + 1) for key in per_it[it][g]] for g in range(len(graphs))])


def sp_hash_features(graphs, hashed, labels=None):
    """One draw of shortest_path_kernel_explicit.py:66-71 -> integer CSR [G, F].  labels None: the key (h_k, h_j, distance) of
    line 71.  labels "node" | "degree": the endpoint class is the joint (label, hash) class, the key of the commented line 67."""
    hashed = O.dense_ranks(hashed)
    if labels is not None:
        lab = O.initial_colours(graphs, labels)
        hashed = O.dense_ranks(lab * (int(hashed.max()) + 1 if hashed.size else 1) + hashed)
    return O.sp_features(with_labels(graphs, hashed), "node")


def hash_features(graphs, bucket, base, iterations=3, labels=None):
    """-> the R per-draw feature matrices for bucket [R, Nv]."""
    return [wl_hash_features(graphs, bk, iterations, labels) if base == "wl" else sp_hash_features(graphs, bk, labels) for bk in bucket]


def columns(features):
    """Columns of the stacked feature matrix that hold a count."""
    return int(sum(int((np.asarray(abs(f).sum(axis=0)).reshape(-1) > 0).sum()) for f in features))


def exact_gram(features):
    """hash_graph_kernel.py:57-66 without its rounding: the integer F F^T of the stacked feature maps, divided by R once."""
    total = sum(O.gram(f) for f in features)
    assert int(np.abs(total).max(initial=0)) < 2 ** 53
    return total.astype(np.float64) / np.float64(len(features))


def hash_gram(graphs, X, V, b, w=1.0, base="wl", iterations=3, labels=None, scale=True, normalize=False):
    Xs = scale_attributes(X)[0] if scale else np.asarray(X, np.float64)
    K = exact_gram(hash_features(graphs, buckets(Xs, V, b, w), base, iterations, labels))
    return O.normalize(K) if normalize else K


def to_attributes(graphs, X, M=None):
    """X [Nv, d] -> the padded [T, M, d] tensor the public function takes."""
    M = max([g[0] for g in graphs] + [1]) if M is None else M
    out = np.zeros((len(graphs), M, X.shape[1]), np.float64)
    at = 0
    for g, (n, _, _) in enumerate(graphs):
        out[g, :n] = X[at:at + n]
        at += n
    return out
