"""Classical graph-kernel baselines of the reference's graph_kernel/gk.py on the device: the Weisfeiler-Lehman subtree kernel
(graphkernel/wl_kernel.py) and the shortest-path kernel (graphkernel/shortest_path_kernel_explicit.py) as exact float64 Gram
matrices, and the nested k-fold SVM of gk.py:243-292 over them: on the host (scikit-learn, the default) or on the device.

    K = wl_subtree_kernel(adjs, num_nodes, node_labels, iterations=3)      # [G, G] float64 on the device, normalised
    K = shortest_path_kernel(adjs, num_nodes, node_labels)
    result = svm_cv(K.cpu().numpy(), y)                                    # 125 SVC fits one after another on the host
    result = svm_cv(K, y, device=True)                                     # the same fits as one batch, K stays on the device

The device route (svm_fit / svm_decision / svm_predict, csrc/svm.hip through ops.svm_smo_batch / svm_decision_batch / svm_vote) is
libsvm's SMO with second-order working-set selection in fp64, one workgroup a problem, without shrinking and without a kernel
cache, in bounded launches; a problem that reaches max_iter raises ops.SvmNotConverged.  Its iterates are a pure function of the
input (the tests restate them in numpy bit for bit); it agrees with SVC to the solver tolerance, not bit for bit (libsvm
keeps its kernel rows in float32), so SVM_DEVICE = False keeps the host route the default.  Up to 4,096 training rows a fit; every
training set must hold every class of y.

The features are computed by csrc/graphkern.hip (ops.wl_refine / wl_rank / wl_runs / sp_features) as runs (column, graph, count),
the Gram by ops.gram_from_runs: columns that occur in one graph on an int64 diagonal, the others on v_mfma_f64_16x16x4_f64.
All sums are sums of non-negative integers below 2^53, so the raw Gram has the bits of the reference's float64 csr.dot and
does not depend on any order; the normalisation (one product, one sqrt, one division in fp64, each correctly rounded on the
device) equals auxiliary_methods.normalize_gram_matrix bit for bit.  Shortest paths are breadth-first searches from every
source in LDS (measured against Floyd-Warshall in the same kernel: 4.4 against 5.8 ms for 20,000 graphs of 50 nodes, 12.9
against 22.5 ms for 2,000 graphs of 128 nodes, profiles/sp_bfs_vs_floyd_warshall.txt).

The adjacency is read as the reference reads it (dataset2graph.py:56-57): entries with row >= col, each one undirected edge
occurrence, a repeated entry a multi-edge; the driver symmetrises them.  Stored values are ignored.

Deviations from the reference
  * Self-loops are dropped.  kGCN preprocessing adds one to every node, and graph_tool's weight of an undirected self-loop
    cannot be checked without graph_tool; when every node has one, the WL partition and the SP distances are the same with
    or without them.
  * Colours are exact multiset classes: a node's new colour is the class of (own colour, sorted multiset of neighbour
    colours), compared exactly (a 128-bit hash orders the rows, equal hashes are verified against the true signatures, and a
    mismatch raises).  The reference rounds sums of log-primes to 10 decimals.
  * svm_cv maps the inner fold positions through idx_train_val; gk.py:264 uses them as global indices and so trains on
    test graphs.
  * The shuffle of the data set is seeded (examples/graph_kernel.py --seed).
  * No cut to 3,000 graphs by default (--limit).

Continuous node attributes: hash_graph_kernel (graphkernel/hash_graph_kernel.py over auxiliary_methods.py:23-36 and the
hashed_attributes argument of both base kernels).  The attribute rows of the existing nodes are scaled to zero mean and unit
variance, projected on R random directions and cut into buckets floor((x . v + b) / w) in fp64 by csrc/hashkern.hip (ops.attr_scale,
ops.lsh_buckets; a stated summation order, nothing fused, so the tests restate them in numpy bit for bit); the base kernel
runs on the buckets' dense ranks and the R feature maps share one Gram.  batched=True takes the R colourings through ONE launch
sequence over the one stored adjacency (ops.wl_refine_copies / wl_rank_copies / wl_runs_copies: one mismatch read-back a
refinement for all draws; ops.sp_features_copies: one breadth-first search a graph for all draws); batched=False runs the draws one
after another through the plain ops and gives the same bits.  Each plain op and its _copies form are one body in ops.py, the
plain one being copies = 1 through its own C entry point; _refine here is the one refinement loop of both routes.
HASH_BATCHED is the measured default (tools/hash_kernel_bench.py).
  Deviations of hash_graph_kernel from the reference
  * K = F F^T / R exactly: the integer Gram over the runs of all draws, divided by R in one fp64 division.
    hash_graph_kernel.py:63-65 rounds sqrt(1 / R) into every count first (measured difference: at most 1.6e-14 relative at R = 20).
  * base="sp" with labels: the endpoint class is the joint (label, hash) class, the key (l_k, h_k, l_j, h_j, distance) of the
    commented shortest_path_kernel_explicit.py:67.  The live line 68 ignores the hashes, so its result is shortest_path_kernel
    itself, R times over.
  * The projections are drawn on the host from np.random.default_rng(seed) (lsh_draws), not from numpy's global state; explicit
    `projections` / `offsets` reproduce any other draw.
  * A column whose values are all equal has variance 0 and becomes 0 (sklearn also treats a variance within rounding of 0 so).
  * base="wl" with labels (use_labels 1 | 2, wl_kernel.py:63-82): label colours and hashed colours are refined separately and
    every iteration counts the joint classes, as the reference does; the joint class is the exact pair, not a hash of it.
Limits: shortest_path_kernel takes graphs of up to 128 nodes and 4,096 distinct labels (a distance is a byte and the key packs
12 + 12 + 8 bits); wl_subtree_kernel up to 4,096 nodes a graph; up to 46,340 graphs a Gram.  hash_graph_kernel: the base kernel's
limits, with base="sp" up to 4,096 (joint) classes in every draw; up to 4,096 attributes a node; R * T * M below 2^31 - 1; a
projected value that is not finite or reaches 2^62 is refused."""
import copy

import numpy as np
import torch

from . import _lib, ops
from .batched_csr import BatchedAdjacency, BatchedCSR

__all__ = ["wl_subtree_kernel", "shortest_path_kernel", "hash_graph_kernel", "lsh_draws", "dense_label_ranks", "dataset_graphs",
           "dataset_attributes", "svm_cv", "svm_fit", "svm_decision", "svm_predict", "SvmBatch",
           "GraphSet"]


def dense_label_ranks(labels):
    """Arbitrary integer labels (negative, up to 2^31 - 1 and beyond) -> (ranks int32 of the same shape, number of distinct
    labels): np.unique(..., return_inverse=True) of the reference."""
    a = np.asarray(labels)
    if a.size and not np.issubdtype(a.dtype, np.integer):
        if not np.all(a == np.floor(a)):
            raise ValueError("node labels must be integers")
    a = a.astype(np.int64)
    uniq, inv = np.unique(a.reshape(-1), return_inverse=True)
    return inv.reshape(a.shape).astype(np.int32), int(uniq.size)


class GraphSet:
    """A data set on the device as the kernels read it: the symmetrised, self-loop-free BatchedCSR, num_nodes [T] and the raw
    node labels / degrees of the nodes that exist (host)."""

    def __init__(self, adjacency, num_nodes, node_labels=None, device="cuda"):
        g, r, c, T, M = _host_entries(adjacency)
        nn = np.asarray(num_nodes, np.int64).reshape(-1)
        if nn.shape[0] != T or (T and (nn.min() < 0 or nn.max() > M)):
            raise ValueError("num_nodes must hold %d values in 0..%d" % (T, M))
        keep = r > c                                     # the lower triangle, without self-loops
        g, r, c = g[keep], r[keep], c[keep]
        if g.size and np.any(r >= nn[g]):
            raise ValueError("an adjacency entry names a node at or past num_nodes of its graph")
        self.T, self.M, self.num_nodes_host = T, M, nn
        self.exists = np.arange(M)[None, :] < nn[:, None]                    # [T, M]
        self.degree = np.bincount(np.r_[g * M + r, g * M + c], minlength=T * M).reshape(T, M)
        self.csr = BatchedCSR.from_arrays(np.r_[g, g], np.r_[r, c], np.r_[c, r], np.ones(2 * g.size, np.float32), T, M, M, device=device)
        self.device = self.csr.device
        self.num_nodes = torch.from_numpy(nn.astype(np.int32)).to(self.device)
        if node_labels is None:
            self.node_labels = None
        else:
            lab = np.zeros((T, M), np.int64)
            for t in range(T):
                row = np.asarray(node_labels[t]).reshape(-1)
                if row.shape[0] < nn[t]:
                    raise ValueError("graph %d: %d labels for %d nodes" % (t, row.shape[0], nn[t]))
                lab[t, :nn[t]] = row[:nn[t]]
            self.node_labels = lab

    def initial_colours(self, labels):
        """-> (device int32 [T*M] dense ranks over the set, -1 where no node exists; number of distinct labels)."""
        if labels == "node":
            if self.node_labels is None:
                raise ValueError('labels="node" needs node_labels')
            raw = self.node_labels
        elif labels == "degree":
            raw = self.degree
        else:
            raise ValueError('labels must be "node" or "degree", got %r' % (labels,))
        ranks, count = dense_label_ranks(raw[self.exists])
        full = np.full((self.T, self.M), -1, np.int32)
        full[self.exists] = ranks
        return torch.from_numpy(full.reshape(-1)).to(self.device), count


def _host_entries(adjacency):
    """-> (graph, row, col int64 arrays of every stored entry, T, M) of channel 0."""
    if isinstance(adjacency, BatchedAdjacency):
        adjacency = adjacency.channels[0]
    if isinstance(adjacency, BatchedCSR):
        a = adjacency
        if a.row_pad != 0 or a.rows != a.cols:
            raise ValueError("a plain square adjacency is required")
        rowptr = a.rowptr.cpu().numpy().astype(np.int64)
        rows = np.repeat(np.arange(a.num_graphs * a.rows, dtype=np.int64), np.diff(rowptr))
        col = a.cv[:, 0].cpu().numpy().astype(np.int64) if a.nnz else np.zeros(0, np.int64)
        return rows // max(a.rows, 1), rows % max(a.rows, 1), col, a.num_graphs, a.rows
    T = len(adjacency)
    gs, rs, cs, M = [], [], [], 0
    for t, chans in enumerate(adjacency):
        m = chans[0]
        idx = np.asarray(m[0], np.int64).reshape(-1, 2)
        if len(m) > 2 and m[2] is not None:
            M = max(M, int(m[2][0]), int(m[2][1]))
        elif idx.size:
            M = max(M, int(idx.max()) + 1)
        gs.append(np.full(idx.shape[0], t, np.int64))
        rs.append(idx[:, 0])
        cs.append(idx[:, 1])
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0, np.int64)  # noqa: E731
    g, r, c = cat(gs), cat(rs), cat(cs)
    if g.size and (min(r.min(), c.min()) < 0 or max(r.max(), c.max()) >= M):
        raise ValueError("an adjacency index lies outside its matrix")
    return g, r, c, T, max(M, 1)


def _as_graph_set(adjacency, num_nodes, node_labels):
    return adjacency if isinstance(adjacency, GraphSet) else GraphSet(adjacency, num_nodes, node_labels)


def _finish(runs, G, normalize, return_gram, chunk_cols):
    col = torch.cat([r[0] for r in runs])
    graph = torch.cat([r[1] for r in runs])
    count = torch.cat([r[2] for r in runs])
    if return_gram:
        return ops.gram_from_runs(col, graph, count, G, chunk_cols=chunk_cols, normalize=normalize)
    import scipy.sparse as sps
    keys = col.cpu().numpy().view(np.uint64)
    uniq, inv = np.unique(keys, return_inverse=True)
    return sps.csr_matrix((count.cpu().numpy().astype(np.int64), (graph.cpu().numpy(), inv.reshape(-1))), shape=(G, max(uniq.size, 1)))


def _refuse_mismatches(info, it, mask):
    mismatches = int(info[1].item())                                  # the read-back
    if mismatches:
        raise _lib.KgcnHipError("wl refinement %d: %d pairs of nodes share a 128-bit key (mask %#x) but differ in their "
                                "signatures; the partition would merge them, refused" % (it + 1, mismatches, mask))


def _refine(gs, col, iterations, hash_mask, copies=None):
    """refine -> rank -> refuse, `iterations` times -> the [iterations + 1] colourings, col first.  copies None: the one
    colouring col [T*M] through the plain ops; otherwise col [copies * T*M] through the copies ops, all copies at once: the one
    read-back a refinement (the mismatch count) serves them all.  A hash collision that merged two signatures raises."""
    mask = ops.HASH_MASK_FULL if hash_mask is None else int(hash_mask)
    out = [col]
    for it in range(int(iterations)):
        if copies is None:
            sorted_nbr, hi, lo = ops.wl_refine(gs.csr, gs.num_nodes, col, mask)
            col, info = ops.wl_rank(gs.csr, gs.num_nodes, col, sorted_nbr, hi, lo)
        else:
            sorted_nbr, hi, lo = ops.wl_refine_copies(gs.csr, gs.num_nodes, col, copies, mask)
            col, info = ops.wl_rank_copies(gs.csr, gs.num_nodes, col, copies, sorted_nbr, hi, lo)
        _refuse_mismatches(info, it, mask)
        out.append(col)
    return out


@torch.no_grad()
def wl_colourings(adjacency, num_nodes=None, node_labels=None, iterations=3, labels="node", hash_mask=None):
    """The colours after every refinement -> ([iterations + 1] device int32 [T, M] tensors, -1 where no node exists; the
    GraphSet).  Raises when a hash collision merged two different signatures (never silently)."""
    gs = _as_graph_set(adjacency, num_nodes, node_labels)
    return [c.view(gs.T, gs.M) for c in _refine(gs, gs.initial_colours(labels)[0], iterations, hash_mask)], gs


@torch.no_grad()
def wl_subtree_kernel(adjacency, num_nodes=None, node_labels=None, iterations=3, labels="node", normalize=True, return_gram=True,
                      chunk_cols=None, hash_mask=None):
    """weisfeiler_lehman_subtree_kernel(graph_db, [], iterations, True, normalize, 1 | 2) of the reference -> the Gram [G, G]
    float64 on the device; return_gram=False: the per-graph feature counts as an integer scipy CSR [G, features] on the host.
    adjacency: a BatchedAdjacency / BatchedCSR or kGCN's adjs[b][ch] COO lists (channel 0), or a GraphSet built once;
    labels="degree" is use_labels == 2.  hash_mask narrows the refinement's hash (tests force collisions with it)."""
    cols, gs = wl_colourings(adjacency, num_nodes, node_labels, iterations, labels, hash_mask)
    runs = [ops.wl_runs(c.reshape(-1), gs.num_nodes, gs.T, gs.M, it << 32) for it, c in enumerate(cols)]
    return _finish(runs, gs.T, normalize, return_gram, chunk_cols)


@torch.no_grad()
def shortest_path_kernel(adjacency, num_nodes=None, node_labels=None, iterations=None, labels="node", normalize=True,
                         return_gram=True, chunk_cols=None):
    """shortest_path_kernel(graph_db, [], True, normalize, 1 | 2) of the reference: every ordered node pair (k, j) of a graph,
    k = j and unreachable pairs included, is the feature (label_k, label_j, distance).  Same arguments as wl_subtree_kernel
    (`iterations` is accepted and unused).  Up to 128 nodes a graph and 4,096 distinct labels: refused beyond, with the reason."""
    gs = _as_graph_set(adjacency, num_nodes, node_labels)
    col, count = gs.initial_colours(labels)
    return _finish([ops.sp_features(gs.csr, gs.num_nodes, col, count)], gs.T, normalize, return_gram, chunk_cols)


HASH_BATCHED = True          # hash_graph_kernel(batched=None): the route tools/hash_kernel_bench.py measured faster
_SP_MAX_CLASSES = 4096


def lsh_draws(seed, hash_iterations, d, sigma=1.0, bin_width=1.0):
    """The R projections of auxiliary_methods.py:25-28 drawn on the host from np.random.default_rng(seed), draw after draw:
    v_r = standard_normal(d) * sigma, b_r = bin_width * random() * sigma -> (V [R, d], b [R]) float64."""
    rng = np.random.default_rng(seed)
    V, b = np.empty((int(hash_iterations), int(d)), np.float64), np.empty(int(hash_iterations), np.float64)
    for r in range(int(hash_iterations)):
        V[r] = rng.standard_normal(int(d)) * sigma
        b[r] = bin_width * rng.random() * sigma
    return V, b


def _attribute_rows(attributes, gs):
    """[T, M', d] float32 / float64 -> the rows of the existing nodes [Nv, d] float64 in graph order (host)."""
    a = np.asarray(attributes)
    if a.dtype not in (np.float32, np.float64):
        raise ValueError("attributes must be float32 or float64, got %s" % a.dtype)
    if a.ndim != 3 or a.shape[0] != gs.T or a.shape[1] < (gs.num_nodes_host.max() if gs.T else 0) or a.shape[2] < 1:
        raise ValueError("attributes must be [%d graphs, at least %d nodes, d >= 1], got %s"
                         % (gs.T, gs.num_nodes_host.max() if gs.T else 0, a.shape))
    if a.shape[2] > ops.LSH_MAX_DIM:
        raise ValueError("%d attributes a node, up to %d" % (a.shape[2], ops.LSH_MAX_DIM))
    rows = a[np.arange(a.shape[1])[None, :] < gs.num_nodes_host[:, None]].astype(np.float64)
    if not np.all(np.isfinite(rows)):
        raise ValueError("attributes hold NaN or Inf at %d of %d existing nodes" % (int((~np.isfinite(rows)).any(axis=1).sum()), len(rows)))
    return np.ascontiguousarray(rows)


def _refuse_classes(count, what):
    if count > _SP_MAX_CLASSES:
        raise _lib.KgcnHipError("hash_graph_kernel: %d %s in one draw, up to %d: the shortest-path key packs (class, class, distance) "
                                "into 12 + 12 + 8 bits; a wider bin_width or fewer labels give fewer classes" % (count, what, _SP_MAX_CLASSES))


@torch.no_grad()
def hash_graph_kernel(adjacency, num_nodes=None, attributes=None, base="wl", node_labels=None, labels=None, hash_iterations=20,
                      wl_iterations=3, bin_width=1.0, sigma=1.0, scale_attributes=True, seed=0, projections=None, offsets=None,
                      normalize=True, return_gram=True, batched=None, chunk_cols=None, hash_mask=None):
    """hash_graph_kernel(graph_db, base_kernel, params, iterations=hash_iterations, lsh_bin_width=bin_width, sigma,
    normalize_gram_matrix=normalize, scale_attributes) of the reference (hash_graph_kernel.py:13-71) -> the Gram [G, G] float64 on the
    device.  attributes [T, M, d] float32 / float64 (promoted to float64; only existing nodes enter the statistics; NaN / Inf is
    refused); base "wl" (wl_iterations refinements) or "sp"; labels None (use_labels == 0: the hashes alone), "node" or "degree"
    (joint (label, hash) classes: see the module text).  projections [R, d] / offsets [R] override the seeded lsh_draws.
    return_gram=False: the integer counts of all draws as a scipy CSR [G, features] (K = F F^T / R).  batched: the module text."""
    if base not in ("wl", "sp"):
        raise ValueError('base must be "wl" or "sp", got %r' % (base,))
    if labels not in (None, "node", "degree"):
        raise ValueError('labels must be None, "node" or "degree", got %r' % (labels,))
    if attributes is None:
        raise ValueError("hash_graph_kernel needs attributes [T, M, d]; without them use wl_subtree_kernel / shortest_path_kernel")
    gs = _as_graph_set(adjacency, num_nodes, node_labels)
    X = _attribute_rows(attributes, gs)
    d = X.shape[1]
    if (projections is None) != (offsets is None):
        raise ValueError("projections and offsets come together")
    if projections is None:
        if int(hash_iterations) < 1:
            raise ValueError("hash_iterations must be at least 1, got %r" % (hash_iterations,))
        projections, offsets = lsh_draws(seed, hash_iterations, d, sigma, bin_width)
    V, b = np.ascontiguousarray(projections, np.float64), np.ascontiguousarray(offsets, np.float64).reshape(-1)
    if V.ndim != 2 or V.shape[0] < 1 or V.shape[1] != d or b.shape[0] != V.shape[0]:
        raise ValueError("projections must be [R >= 1, %d] and offsets [R], got %s and %s" % (d, V.shape, b.shape))
    R, T, M, dev = V.shape[0], gs.T, gs.M, gs.device
    batched = HASH_BATCHED if batched is None else bool(batched)
    if X.shape[0] == 0:                                               # no node: no feature
        if return_gram:
            return torch.zeros((T, T), device=dev, dtype=torch.float64)
        import scipy.sparse as sps
        return sps.csr_matrix((T, 1), dtype=np.int64)

    x = torch.from_numpy(X).to(dev)
    if scale_attributes:
        x = ops.attr_scale(x)[0]
    bucket = ops.lsh_buckets(x, torch.from_numpy(V).to(dev), torch.from_numpy(b).to(dev), bin_width)            # [R, Nv]
    exists = torch.from_numpy(gs.exists.reshape(-1)).to(dev)
    mark = exists.to(torch.int32) - 1                                                                           # [T*M]: 0 / -1
    full = torch.zeros((R, T * M), device=dev, dtype=torch.int64)
    full[:, exists] = bucket
    lab_cols = wl_colourings(gs, iterations=wl_iterations, labels=labels, hash_mask=hash_mask)[0] if labels and base == "wl" else None
    lab0 = gs.initial_colours(labels)[0].to(torch.int64) if labels and base == "sp" else None
    stride = int(wl_iterations) + 1
    runs = []
    if batched:
        markR = mark.repeat(R)
        draw = torch.arange(R, device=dev, dtype=torch.int64)[:, None]
        col = ops.rank_pairs(draw.expand(R, T * M).reshape(-1).contiguous(), full.reshape(-1), markR)[0]     # of (draw, bucket)
        if base == "wl":
            for it, c in enumerate(_refine(gs, col, wl_iterations, hash_mask, copies=R)):
                if lab_cols is not None:                                                          # wl_kernel.py:66-70
                    c = ops.rank_pairs(lab_cols[it].reshape(-1).to(torch.int64).repeat(R), c.to(torch.int64), markR)[0]
                runs.append(ops.wl_runs_copies(c, gs.num_nodes, T, M, R, it << 32, stride << 32))
        else:
            if lab0 is not None:                                      # shortest_path_kernel_explicit.py:67
                col = ops.rank_pairs(((draw << 32) + lab0[None, :]).reshape(-1), col.to(torch.int64), markR)[0]
            c = col.view(R, T * M)                                    # ascending in the draw: every draw's classes are one range
            first = torch.where(c >= 0, c, torch.full_like(c, 2 ** 31 - 1)).amin(dim=1, keepdim=True)
            c = torch.where(c >= 0, c - first, c).contiguous()
            count = int(c.max().item()) + 1
            _refuse_classes(count, "joint (label, hash) classes" if labels else "hash classes")
            runs.append(ops.sp_features_copies(gs.csr, gs.num_nodes, c.reshape(-1), R, count))
    else:
        host = full.view(R, T, M).cpu().numpy()
        for r in range(R):
            one = copy.copy(gs)                                       # the same device adjacency, this draw's buckets as its labels
            one.node_labels = host[r]
            if base == "wl":
                cols = wl_colourings(one, iterations=wl_iterations, labels="node", hash_mask=hash_mask)[0]
                for it, c in enumerate(cols):
                    c = c.reshape(-1)
                    if lab_cols is not None:
                        c = ops.rank_pairs(lab_cols[it].reshape(-1).to(torch.int64), c.to(torch.int64), mark)[0]
                    runs.append(ops.wl_runs(c.contiguous(), gs.num_nodes, T, M, (r * stride + it) << 32))
            else:
                c, count = one.initial_colours("node")
                if lab0 is not None:
                    c, info = ops.rank_pairs(lab0, c.to(torch.int64), mark)
                    count = int(info[0].item())
                _refuse_classes(count, "joint (label, hash) classes" if labels else "hash classes")
                col, graph, n = ops.sp_features(gs.csr, gs.num_nodes, c, count)
                runs.append((col + (r << 32), graph, n))
    if not return_gram:
        return _finish(runs, T, False, False, chunk_cols)
    K = _finish(runs, T, False, True, chunk_cols)
    K = K / torch.tensor(float(R), device=dev, dtype=torch.float64)   # a device divisor: one IEEE division an entry (a host
    return ops.gram_normalize(K) if normalize else K                  # scalar would be multiplied in as its rounded reciprocal)


def dataset_attributes(obj):
    """The node feature tensor of a kGCN data set, "feature" [T, M, F], as hash_graph_kernel's attributes -> float array or None."""
    feat = obj.get("feature")
    return None if feat is None else np.asarray(feat)


def dataset_graphs(obj):
    """What dataset2graph.dataset2graphset reads of a kGCN data set (a joblib dict) -> (adjs[b][0] COO lists, num_nodes [T],
    node_labels per graph or None, label array): "adj" (idx, val, shape) triples or "dense_adj" matrices, "node", "label"."""
    y = np.asarray(obj["label"])
    nodes = obj.get("node")
    adjs, nn = [], []
    if "dense_adj" in obj:
        for a in obj["dense_adj"]:
            a = np.asarray(a)
            r, c = np.nonzero(a.astype(np.int64) != 0)       # dataset2graph.py:28: int(el) != 0
            keep = r >= c
            adjs.append([(np.stack([r[keep], c[keep]], 1).astype(np.int64), np.ones(int(keep.sum()), np.float32), a.shape)])
            nn.append(a.shape[0])
    elif "adj" in obj:
        for a in obj["adj"]:
            idx = np.asarray(a[0], np.int64).reshape(-1, 2)
            adjs.append([(idx, np.ones(idx.shape[0], np.float32), tuple(int(s) for s in a[2]))])
            nn.append(int(a[2][0]))
    else:
        raise KeyError('the data set holds neither "adj" nor "dense_adj"')
    M = max(nn) if nn else 1
    adjs = [[(m[0][0], m[0][1], (M, M))] for m in adjs]
    labels = None if nodes is None else [np.asarray(nodes[t]).reshape(-1)[:nn[t]] for t in range(len(nn))]
    return adjs, np.asarray(nn, np.int32), labels, y


SVM_DEVICE = False           # svm_cv(device=None): the host route (scikit-learn), whose numbers every earlier result holds


class SvmBatch:
    """What svm_fit returns: the fits of F training sets x the C grid, every fit classes (classes - 1) / 2 one-vs-one problems.
    classes: the sorted labels; codes [G] the class index of every row of K (host; labels: the same on the device);
    train: ops.SvmSets, set f * pairs + s = the rows of training set f that belong to pair s, the pair's first class first and +1;
    problem ((f * len(C_grid)) + c) * pairs + s; alpha [P, train.max_rows], rho [P], n_iter [P] on the device; slices: launches."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def problem(self, fit, c, pair=0):
        return (fit * len(self.C_grid) + c) * self.pairs + pair


def _device_gram(K):
    """K as a contiguous float64 device tensor: a device tensor of that form is returned as it is (read in place), an array is uploaded."""
    if not torch.is_tensor(K):
        K = torch.from_numpy(np.ascontiguousarray(K, np.float64))
    if K.is_cuda and K.dtype == torch.float64:
        return K.contiguous()
    return K.to(device="cuda", dtype=torch.float64).contiguous()


@torch.no_grad()
def svm_fit(K, y, train_sets, C_grid, tol=1e-3, max_iter=None, iters_per_launch=None):
    """SVC(kernel="precomputed", C=C, tol=tol).fit(K[tr][:, tr], y[tr]) for every tr of train_sets and every C of C_grid as ONE
    batch on the device (ops.svm_smo_batch: libsvm's SMO in fp64, no shrinking, bounded launches) -> SvmBatch.  K [G, G]: a device
    tensor (read in place) or an array; y [G] any labels.  More than two classes: libsvm's one-vs-one problems, built here.
    A training set that holds one class raises ValueError, as SVC.fit does; so does one that lacks a class of y (SVC would drop
    the class; the batch keeps one class list).  A problem that reaches max_iter raises ops.SvmNotConverged."""
    K = _device_gram(K)
    G = int(K.shape[0])
    y = np.asarray(y).reshape(-1)
    if y.shape[0] != G:
        raise ValueError("y holds %d labels for a %d-row K" % (y.shape[0], G))
    classes, codes = np.unique(y, return_inverse=True)
    codes = codes.reshape(-1).astype(np.int32)
    k = int(classes.shape[0])
    if k > ops.SVM_MAX_CLASSES:
        raise ValueError("%d classes, up to %d" % (k, ops.SVM_MAX_CLASSES))
    C_grid = np.asarray(C_grid, np.float64).reshape(-1)
    pair_list = [(a, b) for a in range(k) for b in range(a + 1, k)]
    sets, signs = [], []
    train_sets = [np.asarray(tr, np.int64).reshape(-1) for tr in train_sets]
    for f, tr in enumerate(train_sets):
        if tr.size and (tr.min() < 0 or tr.max() >= G):
            raise ValueError("training set %d names a row outside 0..%d" % (f, G - 1))
        present = np.unique(codes[tr])
        if present.size < 2:
            raise ValueError("The number of classes has to be greater than one; got %d class (training set %d)" % (present.size, f))
        if present.size < k:
            raise ValueError("training set %d holds %d of the %d classes of y; every training set must hold them all" % (f, present.size, k))
        for a, b in pair_list:                                       # svm.cpp svm_train: the rows of class a, then those of class b
            rows = np.concatenate([tr[codes[tr] == a], tr[codes[tr] == b]])
            sets.append(rows)
            signs.append(np.where(codes[rows] == a, 1, -1))
    train = ops.SvmSets(sets, signs, graphs=G, device=K.device)
    F, nC, pairs = len(train_sets), C_grid.shape[0], len(pair_list)
    fit_of, c_of, pair_of = np.unravel_index(np.arange(F * nC * pairs), (F, nC, pairs)) if F * nC * pairs else (np.zeros(0, np.int64),) * 3
    prob_set, prob_C = fit_of * pairs + pair_of, C_grid[c_of] if nC else np.zeros(0)
    alpha, rho, n_iter, status, slices = ops.svm_smo_batch(K, train, prob_set, prob_C, tol=tol, max_iter=max_iter,
                                                           iters_per_launch=iters_per_launch)
    return SvmBatch(classes=classes, codes=codes, labels=torch.from_numpy(codes).to(K.device), train=train, train_sets=train_sets,
                    C_grid=C_grid, pairs=pairs, pair_list=pair_list, prob_set=prob_set.astype(np.int32), prob_C=prob_C, alpha=alpha,
                    rho=rho, n_iter=n_iter, status=status, slices=slices, tol=float(tol))


def _eval_lists(batch, eval_sets):
    F = len(batch.train_sets)
    if len(eval_sets) != F:
        raise ValueError("eval_sets must hold one entry (an index array or a list of them) for each of the %d training sets" % F)
    out = []
    for e in eval_sets:
        one = isinstance(e, np.ndarray) or (len(e) > 0 and np.isscalar(e[0]))
        out.append([np.asarray(e, np.int64).reshape(-1)] if one else [np.asarray(x, np.int64).reshape(-1) for x in e])
    return out


def _svm_jobs(batch, K, eval_sets):
    """-> (dec flat device, job_out, errors, the evaluation SvmSets, groups [(fit, c, e, first job, evaluation set)]: the jobs of a
    group are its pair problems in libsvm's order)."""
    K = _device_gram(K)
    lists = _eval_lists(batch, eval_sets)
    ev = ops.SvmSets([x for l in lists for x in l], graphs=int(K.shape[0]), device=K.device)
    first = np.concatenate([[0], np.cumsum([len(l) for l in lists])])
    groups, job_prob, job_eval = [], [], []
    for f, l in enumerate(lists):
        for c in range(len(batch.C_grid)):
            for e in range(len(l)):
                groups.append((f, c, e, len(job_prob), int(first[f] + e)))
                for s in range(batch.pairs):
                    job_prob.append(batch.problem(f, c, s))
                    job_eval.append(first[f] + e)
    dec, job_out, errors = ops.svm_decision_batch(K, batch.train, batch.prob_set, batch.alpha, batch.rho, ev, job_prob, job_eval,
                                                  check_errors=False)
    return dec, job_out, errors, ev, groups


def _nested(batch, groups, values):
    out = [[[] for _ in batch.C_grid] for _ in batch.train_sets]
    for (f, c, _, _, _), v in zip(groups, values):
        out[f][c].append(v)
    return out


@torch.no_grad()
def svm_decision(batch, K, eval_sets):
    """decision_function of every fit of `batch` on its evaluation rows: eval_sets[f] an index array, or a list of them (validation,
    test, ...), for training set f -> out[f][c][e], a host float64 array: two classes [rows], scikit-learn's sign (>= 0 predicts
    classes[1]); more classes [rows, pairs], libsvm's one-vs-one values (SVC(decision_function_shape="ovo"))."""
    dec, job_out, errors, ev, groups = _svm_jobs(batch, K, eval_sets)
    ops._svm_refuse_errors(errors, "svm_decision")
    d = dec.cpu().numpy()
    vals = []
    for _, _, _, q, _ in groups:
        block = np.stack([d[job_out[q + s]:job_out[q + s + 1]] for s in range(batch.pairs)], axis=1)
        vals.append(-block[:, 0] if len(batch.classes) == 2 else block)
    return _nested(batch, groups, vals)


@torch.no_grad()
def svm_predict(batch, K, eval_sets, return_correct=False):
    """predict of every fit on its evaluation rows (the decision and vote kernels, one read-back) -> out[f][c][e]: the predicted labels;
    return_correct: also correct[f][c][e], the number of rows whose prediction equals y."""
    dec, job_out, errors, ev, groups = _svm_jobs(batch, K, eval_sets)
    pred, vote_out, counts = ops.svm_vote(dec, job_out, ev, [g[3] for g in groups], [g[4] for g in groups], len(batch.classes),
                                          batch.labels, check_errors=False)
    host = torch.cat([counts, errors]).cpu().numpy()                  # the one read-back: correct counts and both error words
    if host[-1] or host[-2]:
        raise _lib.KgcnHipError("svm_predict: the device found %d descriptors out of range" % int(host[-1] + host[-2]))
    p = pred.cpu().numpy()
    preds = _nested(batch, groups, [batch.classes[p[vote_out[i]:vote_out[i + 1]]] for i in range(len(groups))])
    return (preds, _nested(batch, groups, [int(v) for v in host[:len(groups)]])) if return_correct else preds


def svm_cv(K, y, test_splits=5, C_grid=None, idx_train_val=None, idx_test=None, val_splits=None, device=None, tol=1e-3):
    """The nested KFold / SVC(kernel="precomputed") loop of gk.py:243-292.  For each outer split every C of the
    grid is fitted on each inner training fold; the C with the best mean validation accuracy gives the split's test accuracy
    (the mean over the inner folds, as the reference reports it).  Inner fold positions index idx_train_val (gk.py:264 uses
    them as global indices).  idx_train_val / idx_test: one explicit outer split instead of the KFold.
    device: False the host route (scikit-learn, one fit after another), True the device route: all outer splits x inner folds x C
    are ONE svm_fit, one decision launch and one vote, K a device tensor or an array; None reads SVM_DEVICE.  tol: SVC's tol on
    the host route, the stopping tolerance of the device solver.  The two routes agree to that tolerance, not bit for bit.
    -> {"best_C", "val_acc", "test_acc": per outer split; "mean", "std": of test_acc; "fit_indices": the index array of every fit}."""
    device = SVM_DEVICE if device is None else bool(device)
    y = np.asarray(y).reshape(-1)
    C_grid = np.linspace(1e-4, 10, 5) if C_grid is None else np.asarray(C_grid, np.float64)
    val_splits = test_splits if val_splits is None else val_splits
    if device:
        return _svm_cv_device(K, y, test_splits, C_grid, idx_train_val, idx_test, val_splits, tol)
    from sklearn.metrics import accuracy_score
    from sklearn.model_selection import KFold
    from sklearn.svm import SVC
    K = np.asarray(K.cpu() if torch.is_tensor(K) else K, np.float64)
    outer = _explicit_split(idx_train_val, idx_test) or [(np.asarray(a), np.asarray(b))
                                                         for a, b in KFold(n_splits=test_splits).split(np.arange(K.shape[0]))]
    fit_indices, val, test = [], [], []
    for tv, te in outer:
        for a, b in KFold(n_splits=val_splits).split(tv):
            tr, va = tv[a], tv[b]
            fit_indices.append(tr)
            base = K[:, tr]
            fits = [SVC(kernel="precomputed", C=float(C), tol=tol).fit(base[tr, :], y[tr]) for C in C_grid]
            val.append([accuracy_score(y[va], clf.predict(base[va, :])) for clf in fits])
            test.append([accuracy_score(y[te], clf.predict(base[te, :])) for clf in fits])
    return _cv_summary(C_grid, val, test, fit_indices, val_splits)


def _explicit_split(idx_train_val, idx_test):
    """svm_cv's outer splits [(training-and-validation rows, test rows)] when one is given; None: the route's own k-fold makes them."""
    return None if idx_train_val is None else [(np.asarray(idx_train_val, np.int64), np.asarray(idx_test, np.int64))]


def _cv_summary(C_grid, val, test, fit_indices, val_splits):
    """val, test [fit][C]: the accuracies of every fit, the val_splits inner folds of an outer split one after another -> what
    svm_cv returns: per outer split the C of the best mean validation accuracy and the two means at it; mean and std of test_acc."""
    out = {"best_C": [], "val_acc": [], "test_acc": [], "fit_indices": fit_indices}
    for o in range(0, len(val), val_splits):
        v, t = np.mean(val[o:o + val_splits], axis=0), np.mean(test[o:o + val_splits], axis=0)
        best = int(np.argmax(v))
        out["best_C"].append(float(C_grid[best]))
        out["val_acc"].append(float(v[best]))
        out["test_acc"].append(float(t[best]))
    out["mean"] = float(np.mean(out["test_acc"]))
    out["std"] = float(np.std(out["test_acc"]))
    return out


def _kfold(m, splits):
    """KFold(n_splits=splits).split(range(m)) without shuffling -> [(train positions, test positions)]."""
    if not 2 <= splits <= m:
        raise ValueError("%d splits of %d samples" % (splits, m))
    sizes = np.full(splits, m // splits, np.int64)
    sizes[:m % splits] += 1
    stops = np.cumsum(sizes)
    return [(np.r_[0:s - z, s:m].astype(np.int64), np.arange(s - z, s, dtype=np.int64)) for s, z in zip(stops, sizes)]


def _svm_cv_device(K, y, test_splits, C_grid, idx_train_val, idx_test, val_splits, tol):
    K = _device_gram(K)
    trains, evals = [], []
    for tv, te in _explicit_split(idx_train_val, idx_test) or _kfold(int(K.shape[0]), test_splits):
        for a, b in _kfold(len(tv), val_splits):
            trains.append(tv[a])
            evals.append([tv[b], te])
    batch = svm_fit(K, y, trains, C_grid, tol=tol)
    _, correct = svm_predict(batch, K, evals, return_correct=True)
    val, test = ([[correct[f][c][e] / len(evals[f][e]) for c in range(len(C_grid))] for f in range(len(trains))] for e in (0, 1))
    return _cv_summary(C_grid, val, test, list(trains), val_splits)
