"""fp64 numpy restatement of `kgcn visualize` for the link-prediction model (kgcn/visualization.py:289-439, cal_feature_IG_for_kg
and KnowledgeGraphVisualizer) on model_py/gcn.py: integrated gradients of one label row's score (model.score[target] = s1), of its
cost (model.loss[target]) or of one entry of the prediction with respect to the embedded layer.  Test infrastructure only.

  literal       the reference loop: for every step k a full forward of linkpred_oracle.node_rows on alpha_k E, the backward chain
                of linkpred_oracle.model_grads seeded by the target, IG += grad * E * w_k
  restructured  the algebra the HIP kernel implements: layer 1 is affine in alpha, layer 2 is stashed once for all
                targets, a target seeds at most four rows, and the sum over k moves inside A^T and W1

A target is (a, b, a', b'): score mode reads (a, b) only (a', b' = -1), loss mode all four (label columns 0, 2, 3, 5)."""
import numpy as np
import scipy.sparse as sp

import linkpred_oracle as LO

SCORE, LOSS = 0, 1


def reference_scales(K):
    """visualization.py:328-337: alpha_k = (k + 1) / K, w_k = 1 / K."""
    return np.arange(1, K + 1, dtype=np.float64) / K, np.full(K, 1.0 / K)


def _seeds(H, target, mode):
    """-> (score, [(seed row, partner row, coefficient)]): d score / d H[seed] += coefficient H[partner]."""
    a, b, a2, b2 = (int(v) for v in target)
    s1 = float(H[a] @ H[b])
    if mode == SCORE:
        return s1, [(a, b, 1.0), (b, a, 1.0)]
    s2 = float(H[a2] @ H[b2])
    c = float(LO.pair_dcost(s1, s2, "gcn"))
    return s1 - s2, [(a, b, c), (b, a, c), (a2, b2, -c), (b2, a2, -c)]


def literal(params, A, target, mode, scales, weights):
    """-> dict ig [N, De], u [N, C] (= sum_k w_k dZ1_k), node_ig [N] (= ig.sum(-1)), score [K]."""
    E = np.asarray(params["embedding"], np.float64)
    ig = np.zeros_like(E)
    u = None
    score = np.zeros(len(scales))
    for k, (al, wk) in enumerate(zip(scales, weights)):
        p = dict(params, embedding=al * E)
        H, (_, z1, h1, z2) = LO.node_rows(p, "gcn", A)
        score[k], seeds = _seeds(H, target, mode)
        dH = np.zeros_like(H)
        for s, q, c in seeds:
            dH[s] += c * H[q]
        dz2 = dH * (z2 > 0)
        dy2 = A.T @ dz2
        dz1 = (dy2 @ np.asarray(params["w2"], np.float64).T) * (z1 > 0)
        dy1 = A.T @ dz1
        grad = dy1 @ np.asarray(params["w1"], np.float64).T
        ig += grad * E * wk
        u = wk * dz1 if u is None else u + wk * dz1
    return dict(ig=ig, u=u, node_ig=ig.sum(-1), score=score)


def stash(params, A, scales):
    """What is computed once for all targets: P = E W1, G1 = A P, r = row sums of A, H2 [K, N, C]."""
    E = np.asarray(params["embedding"], np.float64)
    w1, w2 = np.asarray(params["w1"], np.float64), np.asarray(params["w2"], np.float64)
    b1, b2 = np.asarray(params["b1"], np.float64).reshape(-1), np.asarray(params["b2"], np.float64).reshape(-1)
    P = E @ w1
    G1 = A @ P
    r = np.asarray(A.sum(1)).reshape(-1)
    z1 = [al * G1 + np.outer(r, b1) for al in scales]
    z2 = [A @ (np.maximum(z, 0.0) @ w2 + b2) for z in z1]
    return dict(E=E, P=P, G1=G1, r=r, b1=b1, w1=w1, w2=w2, z1=np.stack(z1), z2=np.stack(z2), H2=np.maximum(np.stack(z2), 0.0))


def restructured(params, A, target, mode, scales, weights, st=None):
    """Same outputs as literal(), by the formulas of the kernel; every (seed, partner) entry is handled on its own."""
    st = stash(params, A, scales) if st is None else st
    csr = sp.csr_matrix(A)
    N, C = st["G1"].shape
    u = np.zeros((N, C))
    score = np.zeros(len(scales))
    for k, (al, wk) in enumerate(zip(scales, weights)):
        H = st["H2"][k]
        score[k], seeds = _seeds(H, target, mode)
        for s, q, c in seeds:
            dz2 = c * H[q] * (H[s] > 0)
            v = dz2 @ st["w2"].T
            for e in range(csr.indptr[s], csr.indptr[s + 1]):
                i = csr.indices[e]
                u[i] += wk * csr.data[e] * v * (al * st["G1"][i] + st["r"][i] * st["b1"] > 0)
    node_ig = np.zeros(N)
    for i in np.nonzero(np.abs(u).sum(1))[0]:
        for e in range(csr.indptr[i], csr.indptr[i + 1]):
            j = csr.indices[e]
            node_ig[j] += csr.data[e] * float(u[i] @ st["P"][j])
    ig = st["E"] * ((A.T @ u) @ st["w1"].T)
    return dict(ig=ig, u=u, node_ig=node_ig, score=score)


def score_at(params, A, target, mode, alpha):
    """The attributed quantity at scale alpha: s1 (score mode) or the cost (loss mode)."""
    H, _ = LO.node_rows(dict(params, embedding=alpha * np.asarray(params["embedding"], np.float64)), "gcn", A)
    a, b, a2, b2 = (int(v) for v in target)
    s1 = float(H[a] @ H[b])
    if mode == SCORE:
        return s1
    return float(LO.pair_cost(s1, float(H[a2] @ H[b2]), "gcn"))


def node_partner(params, A, t):
    """visualization.py:429-431: argmax_j (H H^T)[t, j] at alpha = 1."""
    H, _ = LO.node_rows(params, "gcn", A)
    return int(np.argmax(H @ H[t]))


# ---- distmult / ip: the score is bilinear in the table ---------------------------------------------------------------------
def literal_table(E, w, a, b, scales, weights):
    """The reference loop for s = sum_d e_a e_b w (w = 1: ip) with respect to the table -> ig [N, D]."""
    E = np.asarray(E, np.float64)
    w = np.ones(E.shape[1]) if w is None else np.asarray(w, np.float64)
    ig = np.zeros_like(E)
    for al, wk in zip(scales, weights):
        X = al * E
        g = np.zeros_like(E)
        g[a] += X[b] * w
        g[b] += X[a] * w
        ig += g * E * wk
    return ig


def closed_table(E, w, a, b, scales, weights):
    """IG[a] = e_a w e_b sum_k w_k alpha_k, likewise b (a == b: both land on the one row)."""
    E = np.asarray(E, np.float64)
    w = np.ones(E.shape[1]) if w is None else np.asarray(w, np.float64)
    f = float(np.dot(scales, weights))
    ig = np.zeros_like(E)
    ig[a] += E[a] * w * E[b] * f
    ig[b] += E[b] * w * E[a] * f
    return ig


# ---- shared test inputs ------------------------------------------------------------------------------------------------------
def make_graph(N=70, seed=5):
    """A directed N-node graph (idx [nnz, 2] sorted by row then column, val [nnz]): row 0 is a hub with N - 4 entries (wider
    than a wave at N = 70), row 1 holds its self loop only, every other row its self loop and up to four other columns;
    values in {0.5, 1, 2}; A != A^T."""
    rng = np.random.RandomState(seed)
    ent = {(0, int(c)) for c in range(N - 4)} | {(1, 1)}
    for r in range(2, N):
        ent.add((r, r))
        for c in rng.choice(N, 4, replace=False):
            ent.add((r, int(c)))
    idx = np.array(sorted(ent), np.int64)
    val = rng.choice([0.5, 1.0, 2.0], len(idx))
    return idx, val


def grid_params(N, De=16, C=128, seed=7):
    """Parameters on a dyadic grid (all multiples of 1/8): with dyadic scales every pre-activation of both layers is exact in
    fp32, so no relu mask can differ between the fp32 kernels and the fp64 oracle."""
    rng = np.random.RandomState(seed)

    def sparse(shape, per_col, choices):
        w = np.zeros(shape)
        for c in range(shape[1]):
            w[rng.choice(shape[0], per_col, replace=False), c] = rng.choice(choices, per_col)
        return w
    return dict(embedding=rng.choice([-1, 0, 0, 1], (N, De)) / 8.0,
                w1=sparse((De, C), 2, [-1.0, 1.0]), b1=rng.choice([-1, 0, 0, 0], C) / 8.0,
                w2=sparse((C, C), 2, [-1.0, 1.0]), b2=rng.choice([-1, 0, 0, 0], C) / 8.0)


def random_params(N, De=16, C=128, seed=11):
    """Off-grid parameters, small enough that the ranking cost of a label row is not saturated at scale 1."""
    rng = np.random.RandomState(seed)
    return dict(embedding=rng.uniform(-0.3, 0.3, (N, De)), w1=0.5 * rng.standard_normal((De, C)) / np.sqrt(De),
                b1=0.03 * rng.standard_normal(C), w2=0.12 * rng.standard_normal((C, C)) / np.sqrt(C), b2=0.03 * rng.standard_normal(C))
