"""fp64 numpy restatement of knowledge-graph link prediction (sample_kg/network_prediction of the reference): the preprocessing
that builds the label lists (script/preprocessing_link_pred.py), the label-batch feed (kgcn/feed.py), the three models
model_py/{gcn,distmult,ip}.py with their ranking loss and gradients, and TF's Adam update.  Test infrastructure only."""
import numpy as np

from vae_oracle import philox4x64_10

LOG_EPS = 1e-10
GAMMA = 0.1


# ---- preprocessing (script/preprocessing_link_pred.py) ------------------------------------------------------------------
def load_graph(lines, labels):
    """:8-42 for 2- and 3-column lines -> (edges, nodes, labels); self loops skipped."""
    edges, nodes = set(), set()
    for line in lines:
        arr = line.strip().split("\t")
        if len(arr) == 2:
            arr = [arr[0], "interaction", arr[1]]
        if arr[1] not in labels:                         # :20-22, :31-32
            labels[arr[1]] = len(labels)
        if arr[0] != arr[2]:                             # :23-25, :33-35
            edges.add((arr[0], arr[1], arr[2]))
        nodes.add(arr[0])                                # :28-29, :38-39
        nodes.add(arr[2])
    return edges, nodes, labels


def sample_neg_list(target_nodes, train_target_edges, n):
    """:44-56"""
    out = []
    i_list = np.random.choice(target_nodes, n)
    j_list = np.random.choice(target_nodes, n)
    s = set(train_target_edges)
    for i, j in zip(i_list, j_list):
        if (i, 0, j) not in s:
            out.append((i, 0, j))
    return out


def build_label_list(target_nodes, train_target_edges, m):
    """:58-75: positives in order (reshuffled in place each time they run out), negatives in lists of up to 100."""
    label_list, pi, ni, neg = [], 0, 0, [None]
    for i in range(m):
        if i % len(neg) == 0:
            neg = sample_neg_list(target_nodes, train_target_edges, 100)
            ni = 0
        if pi == len(train_target_edges):
            np.random.shuffle(train_target_edges)
            pi = 0
        label_list.append(train_target_edges[pi] + neg[ni])
        ni += 1
        pi += 1
    return label_list


def build_adjs(base_edges, self_edges, node_num):
    """:77-87 -> (idx [nnz, 2] sorted, val ones, shape)."""
    e = sorted(list(set((a[0], a[2]) for a in base_edges)) + [(a[0], a[2]) for a in self_edges])
    return np.array(e, np.int64), np.ones(len(e), np.int64), np.array((node_num, node_num))


def preprocess(train_lines, test_lines, seed):
    """The __main__ block (:90-170) for --train / --test files under np.random.seed(seed) -> dict of the .jbl arrays.  The
    block iterates Python sets of strings, whose order changes with the interpreter's hash seed; here (and in
    tests/golden/make_golden_linkpred.py) the edge and node lists are sorted first, so the draws are reproducible."""
    np.random.seed(seed)
    labels = {"negative": 0, "self": 1}
    train_edges, train_nodes, labels = load_graph(train_lines, labels)
    test_edges, test_nodes, labels = load_graph(test_lines, labels)
    all_nodes = sorted(train_nodes | test_nodes)
    mp = {el: i for i, el in enumerate(all_nodes)}
    conv = lambda es: [(mp[e[0]], labels[e[1]], mp[e[2]]) for e in es]
    train_edges, test_edges = sorted(conv(train_edges)), sorted(conv(test_edges))
    target_nodes = sorted(mp[e] for e in (train_nodes | test_nodes))
    self_edges = [(i, labels["self"], i) for i in range(len(all_nodes))]
    label_list = build_label_list(target_nodes, train_edges, len(train_edges))
    test_label_list = build_label_list(target_nodes, test_edges, len(test_edges))
    idx, val, shape = build_adjs(train_edges, self_edges, len(all_nodes))
    return dict(adj_idx=idx, adj_val=val, node_num=len(all_nodes), label_list=np.array([label_list], np.int64),
                test_label_list=np.array([test_label_list], np.int64))


# ---- feed (kgcn/feed.py:34-59) -------------------------------------------------------------------------------------------
def draw_indices(seed, step, rows, K):
    """The device's bias-free draw: Philox4x64-10, key (seed, 0), counter (row, step, round, 0); Lemire's multiply-shift on the
    words in order, a word rejected when (w K) mod 2^64 < 2^64 mod K."""
    t = (2 ** 64 - K) % K
    out = np.empty(len(rows), np.int64)
    for n, row in enumerate(rows):
        r, got = 0, None
        while got is None:
            ctr = np.array([[row, step % 2 ** 64, r, 0]], np.uint64)
            words = philox4x64_10(ctr, np.array([[seed % 2 ** 64, 0]], np.uint64))[0]
            for wd in words:
                m = int(wd) * K
                if m % 2 ** 64 >= t:
                    got = m >> 64
                    break
            r += 1
        out[n] = got
    return out


def assemble(label_list, perm, negatives, L, seed, step):
    """Window (step mod floor(M / L)) of the permuted list, col 3 := col 0, col 5 := a drawn negative (feed.py:41-59)."""
    M = len(label_list)
    j = step % (M // L)
    src = np.arange(j * L, j * L + L) if perm is None else np.asarray(perm)[j * L:j * L + L]
    rows = np.array(label_list, np.int64)[src].copy()
    rows[:, 3] = rows[:, 0]
    rows[:, 5] = np.asarray(negatives)[draw_indices(seed, step, range(L), len(negatives))]
    return rows


# ---- loss (model_py/*.py) ------------------------------------------------------------------------------------------------
def scores(h, rows, mode, w=None):
    """pred0..pred3 = gather(prediction, cols 0, 2, 3, 5); s = sum h h' (gcn.py:53-54, ip.py:46-47 before the batch sum) or
    sum h h' w[r] (layers.py:321-325 DistMult.compute_score)."""
    h = np.asarray(h, np.float64)
    p0, p1, p2, p3 = (h[rows[:, c]] for c in (0, 2, 3, 5))
    if mode == "distmult":
        w = np.asarray(w, np.float64)
        return (p0 * p1 * w[rows[:, 1]]).sum(1), (p2 * p3 * w[rows[:, 4]]).sum(1)
    return (p0 * p1).sum(1), (p2 * p3).sum(1)


def pair_cost(s1, s2, mode):
    """gcn.py:59-61: -log(sigmoid(s1 - s2) + 1e-10); distmult.py:55-58 / ip.py:48-51: -log(1 / (1 + exp(s2 - s1 + 0.1)) + 1e-10)."""
    with np.errstate(over="ignore"):
        if mode == "gcn":
            y = 1.0 / (1.0 + np.exp(-(s1 - s2)))
        else:
            y = 1.0 / (1.0 + np.exp(s2 - s1 + GAMMA))
    return -np.log(y + LOG_EPS)


def pair_dcost(s1, s2, mode, f32_limit=True):
    """d cost / d s1 (= -d cost / d s2) as TF differentiates the expression (Sigmoid: y (1 - y); Reciprocal: -y^2; Log: 1/x).
    f32_limit: where exp(s2 - s1 + 0.1) overflows fp32 the derivative is 0 (TF's 0 * inf = NaN is replaced by its limit)."""
    s1, s2 = np.asarray(s1, np.float64), np.asarray(s2, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        if mode == "gcn":
            y = 1.0 / (1.0 + np.exp(-(s1 - s2)))
            return -(y * (1.0 - y)) / (y + LOG_EPS)
        x = s2 - s1 + GAMMA
        e = np.exp(x)
        out = 1.0 / (1.0 + e)
        g = -(out * out * e) / (out + LOG_EPS)
        if f32_limit:
            g = np.where(x > np.log(np.finfo(np.float32).max), 0.0, g)
        return g


def loss(s1, s2, mode):
    """-> dict cost_opt, cost_sum, correct_count (gcn.py:59-70; ip: one cost of the batch sums, correct = [S1 > S2])."""
    if mode == "ip":
        S1, S2 = s1.sum(), s2.sum()
        c = float(pair_cost(S1, S2, mode))
        return dict(cost_opt=c, cost_sum=c, correct_count=float(S1 > S2), S1=S1, S2=S2)
    c = pair_cost(s1, s2, mode)
    return dict(cost_opt=c.mean(), cost_sum=c.sum(), correct_count=float((s1 > s2).sum()))


def upstream(s1, s2, mode, g_opt=1.0, g_sum=0.0):
    """a_i = d (g_opt cost_opt + g_sum cost_sum) / d s1_i."""
    L = len(s1)
    if mode == "ip":
        return np.full(L, (g_opt + g_sum) * float(pair_dcost(s1.sum(), s2.sum(), mode)))
    return (g_opt / L + g_sum) * pair_dcost(s1, s2, mode)


def loss_grads(h, rows, mode, w=None, g_opt=1.0, g_sum=0.0):
    """-> (dh [N, D], dw [R, D] or None) of the loss; vectorised (np.add.at) form."""
    h = np.asarray(h, np.float64)
    s1, s2 = scores(h, rows, mode, w)
    a = upstream(s1, s2, mode, g_opt, g_sum)[:, None]
    ww = np.asarray(w, np.float64) if mode == "distmult" else None
    w1 = ww[rows[:, 1]] if ww is not None else 1.0
    w4 = ww[rows[:, 4]] if ww is not None else 1.0
    h0, h2, h3, h5 = (h[rows[:, c]] for c in (0, 2, 3, 5))
    dh = np.zeros_like(h)
    np.add.at(dh, rows[:, 0], a * h2 * w1)
    np.add.at(dh, rows[:, 2], a * h0 * w1)
    np.add.at(dh, rows[:, 3], -a * h5 * w4)
    np.add.at(dh, rows[:, 5], -a * h3 * w4)
    dw = None
    if ww is not None:
        dw = np.zeros_like(ww)
        np.add.at(dw, rows[:, 1], a * h0 * h2)
        np.add.at(dw, rows[:, 4], -a * h3 * h5)
    return dh, dw


# ---- models ----------------------------------------------------------------------------------------------------------------
def dense_adj(adj_idx, adj_val, N):
    import scipy.sparse as sp
    return sp.csr_matrix((np.asarray(adj_val, np.float64), (adj_idx[:, 0], adj_idx[:, 1])), shape=(N, N))


def node_rows(params, mode, A=None):
    """-> (H, cache): the embedding table (distmult, ip) or relu(A (relu(A (E W1 + b1)) W2 + b2)) (gcn.py:41-46; kgcn
    GraphConv = A (X W + b))."""
    E = np.asarray(params["embedding"], np.float64)
    if mode != "gcn":
        return E, None
    z1 = A @ (E @ params["w1"] + params["b1"].reshape(1, -1))
    h1 = np.maximum(z1, 0.0)
    z2 = A @ (h1 @ params["w2"] + params["b2"].reshape(1, -1))
    return np.maximum(z2, 0.0), (E, z1, h1, z2)


def model_grads(params, mode, rows, A=None, g_opt=1.0):
    """-> (loss dict, gradient dict of every parameter) for one assembled batch."""
    H, cache = node_rows(params, mode, A)
    w = params.get("w")
    s1, s2 = scores(H, rows, mode, w)
    res = loss(s1, s2, mode)
    dH, dw = loss_grads(H, rows, mode, w, g_opt, 0.0)
    g = {}
    if dw is not None:
        g["w"] = dw
    if mode != "gcn":
        g["embedding"] = dH
        return res, g
    E, z1, h1, z2 = cache
    dz2 = dH * (z2 > 0)
    dy2 = A.T @ dz2
    g["w2"], g["b2"] = h1.T @ dy2, dy2.sum(0)
    dz1 = (dy2 @ params["w2"].T) * (z1 > 0)
    dy1 = A.T @ dz1
    g["w1"], g["b1"] = E.T @ dy1, dy1.sum(0)
    g["embedding"] = dy1 @ params["w1"].T
    return res, g


def tf_adam(p, g, m, v, t, lr, b1=0.9, b2=0.999, eps=1e-8):
    """tf.train.AdamOptimizer: lr_t = lr sqrt(1 - b2^t) / (1 - b1^t), p -= lr_t m / (sqrt(v) + eps), t counted from 1."""
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    lr_t = lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t)
    return p - lr_t * m / (np.sqrt(v) + eps), m, v
