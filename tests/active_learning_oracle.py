"""numpy fp64 restatement of csrc/labelprop.hip in the orders include/kgcn_hip.h states: the RBF affinity by scikit-learn's formula,
the degrees, the propagation iterates with their convergence sums, the finish, the five uncertainty scores, the stable
selection, and the loops of kgcn_amd/active_learning.py built on them.  Given the same W the degrees, iterates and finish are the
device's bit for bit (every sum below is written out in its order; nothing is left to numpy's pairwise summation); the affinity
itself and the scores (device exp / log, the matrix pipe's internal order) are compared by tolerance."""
import numpy as np

BLOCK_ROWS = 32              # KGCN_LP_BLOCK_ROWS
PROPAGATION, SPREADING = 0, 1
RUNNING, CONVERGED, MAX_ITER = 0, 1, 2
SCORES = {"E": 0, "LC_MEAN": 1, "MS_MEAN": 2, "LC_TASKS": 3, "MS_TASKS": 4}
_LANE = np.arange(64)


def rbf_affinity(X, gamma):
    """sklearn.metrics.pairwise.rbf_kernel(X, gamma=gamma) as the header writes it: exp(-gamma max(0, (|x_i|^2 + |x_j|^2) - 2 x_i.x_j)),
    the diagonal distance forced to 0."""
    X = np.asarray(X, np.float64)
    norms = np.zeros(X.shape[0])
    for k in range(X.shape[1]):
        norms = norms + X[:, k] * X[:, k]
    dist = (norms[:, None] + norms[None, :]) - 2.0 * (X @ X.T)
    dist = np.maximum(dist, 0.0)
    np.fill_diagonal(dist, 0.0)
    return np.exp(-gamma * dist)


def _lane_tree(acc):
    """acc [rows, 64, ...] -> [rows, ...]: v_l = v_l + v_(l ^ off) for off = 32 .. 1."""
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, _LANE ^ off]
    return acc[:, 0]


def product(W, G):
    """raw [n, K] = sum_j W_ij G_jc: lane l adds the rounded products of j = l, l + 64, ... ascending from +0.0, then the lane tree."""
    n, K = G.shape
    chunks = -(-n // 64)
    Wp = np.zeros((n, chunks * 64))
    Wp[:, :n] = W
    Gp = np.zeros((chunks * 64, K))
    Gp[:n] = G
    acc = np.zeros((n, 64, K))
    for c in range(chunks):
        acc = acc + Wp[:, c * 64:(c + 1) * 64, None] * Gp[None, c * 64:(c + 1) * 64, :]
    return _lane_tree(acc)


def degrees(W):
    """(s, d): the row sums of W with and without the diagonal term (replaced by +0.0), in the order of product()."""
    ones = np.ones((W.shape[0], 1))
    W0 = W.copy()
    np.fill_diagonal(W0, 0.0)
    return product(W, ones)[:, 0], product(W0, ones)[:, 0]


def _columns_sum(V, c0, c1):
    acc = np.zeros(V.shape[0])
    for c in range(c0, c1):
        acc = acc + V[:, c]
    return acc


def _task_sums(delta):
    """delta [n, T] -> [T]: rows inside a block of BLOCK_ROWS in order from +0.0, then the blocks in order from +0.0."""
    n, T = delta.shape
    blocks = -(-n // BLOCK_ROWS)
    d = np.zeros((blocks * BLOCK_ROWS, T))
    d[:n] = delta
    d = d.reshape(blocks, BLOCK_ROWS, T)
    part = np.zeros((blocks, T))
    for r in range(BLOCK_ROWS):
        part = part + d[:, r]
    total = np.zeros(T)
    for b in range(blocks):
        total = total + part[b]
    return total


def onehot(labels, task_col):
    labels = np.asarray(labels)
    n, T = labels.shape
    F = np.zeros((n, int(task_col[-1])))
    for t in range(T):
        for c in range(task_col[t], task_col[t + 1]):
            F[:, c] = labels[:, t] == c - task_col[t]
    return F


def propagate(W, scale, labels, task_col, variant, alpha=0.2, tol=1e-3, max_iter=1000, keep=False):
    """-> dict(F: the distributions before the finish, n_iter [T], status [T], sums: the convergence sum of every check, iterates
    when keep).  scale = s (propagation) or d (spreading) of degrees()."""
    labels = np.asarray(labels)
    n, T = labels.shape
    K = int(task_col[-1])
    Y = onehot(labels, task_col)
    F = Y.copy()
    if variant == SPREADING:
        q = np.where(scale == 0.0, 1.0, np.sqrt(scale))
        Wm = W.copy()
        np.fill_diagonal(Wm, 0.0)
        Ystat = Y * (1.0 - alpha)
    else:
        Wm = W
    status, n_iter = np.zeros(T, np.int32), np.zeros(T, np.int32)
    delta = np.stack([_columns_sum(F, task_col[t], task_col[t + 1]) for t in range(T)], axis=1)
    sums, iterates, k = [], [], 0
    while True:
        total = _task_sums(delta)
        sums.append(total)
        for t in range(T):
            if status[t] == RUNNING:
                if k >= max_iter:
                    status[t], n_iter[t] = MAX_ITER, max_iter
                elif total[t] < tol:
                    status[t], n_iter[t] = CONVERGED, k
        if not np.any(status == RUNNING):
            break
        raw = product(Wm, F / q[:, None] if variant == SPREADING else F)
        Fn, delta = F.copy(), np.zeros((n, T))
        for t in range(T):
            if status[t] != RUNNING:
                continue
            c0, c1 = task_col[t], task_col[t + 1]
            if variant == SPREADING:
                Fn[:, c0:c1] = alpha * (raw[:, c0:c1] / q[:, None]) + Ystat[:, c0:c1]
            else:
                V = raw[:, c0:c1] / scale[:, None]
                norm = _columns_sum(V, 0, c1 - c0)
                norm[norm == 0.0] = 1.0
                Fn[:, c0:c1] = np.where((labels[:, t] >= 0)[:, None], Y[:, c0:c1], V / norm[:, None])
            delta[:, t] = _columns_sum(np.abs(Fn - F), c0, c1)
        F = Fn
        k += 1
        if keep:
            iterates.append(F)
    return {"F": F, "n_iter": n_iter, "status": status, "sums": np.array(sums), "iterates": iterates, "steps": k}


def finish(F, task_col):
    out = np.empty_like(F)
    for t in range(len(task_col) - 1):
        c0, c1 = task_col[t], task_col[t + 1]
        norm = _columns_sum(F, c0, c1)
        norm[norm == 0.0] = 1.0
        out[:, c0:c1] = F[:, c0:c1] / norm[:, None]
    return out


def _entr(p):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(np.isnan(p), p, np.where(p > 0, -p * np.log(np.where(p > 0, p, 1.0)), np.where(p == 0, 0.0, -np.inf)))


def scores(dist, task_col, cand):
    """[5, m] scores of the rows cand of dist (SCORES names the rows)."""
    P = dist[np.asarray(cand, np.int64)]
    m, T = P.shape[0], len(task_col) - 1
    widths = np.diff(task_col)
    E, conf, margins = np.zeros(m), np.zeros(m), np.zeros(m)
    with np.errstate(divide="ignore", invalid="ignore"):
        for t in range(T):
            c0, c1 = task_col[t], task_col[t + 1]
            total = _columns_sum(P, c0, c1)
            E = E + _columns_sum(_entr(P[:, c0:c1] / total[:, None]), 0, c1 - c0)
            top = np.sort(P[:, c0:c1], axis=1)
            conf = conf + top[:, -1]
            margins = margins + (top[:, -1] if c1 - c0 == 1 else top[:, -1] - top[:, -2])
    out = np.full((5, m), np.nan)
    out[SCORES["E"]], out[SCORES["LC_TASKS"]], out[SCORES["MS_TASKS"]] = E, conf / T, margins
    if np.all(widths == widths[0]):
        mean = np.zeros((m, widths[0]))
        for t in range(T):
            mean = mean + P[:, task_col[t]:task_col[t + 1]]
        mean = np.sort(mean / T, axis=1)
        out[SCORES["LC_MEAN"]] = 1.0 - mean[:, -1]
        if widths[0] >= 2:
            out[SCORES["MS_MEAN"]] = mean[:, -1] - mean[:, -2]
    return out


def select(score, k, largest, taking_part=None):
    """Positions in the order of a stable ascending sort with NaN last: its last k (largest) or first k, among those taking part."""
    score = np.asarray(score, np.float64)
    pos = np.arange(score.shape[0]) if taking_part is None else np.flatnonzero(taking_part)
    order = pos[np.argsort(score[pos], kind="stable")]          # numpy sorts NaN last; stable keeps positions ascending among equals
    return order[-k:] if largest else order[:k]


# ---- the drivers' loops ------------------------------------------------------------------------------------------------------------
def encode(Y):
    """Y [n, T] with -1 = unlabelled -> (labels [n, T] class indices, classes per task, task_col)."""
    Y = np.asarray(Y)
    labels, classes, task_col = np.full(Y.shape, -1, np.int32), [], [0]
    for t in range(Y.shape[1]):
        cl = np.unique(Y[:, t])
        cl = cl[cl != -1]
        classes.append(cl)
        for c, v in enumerate(cl):
            labels[Y[:, t] == v, t] = c
        task_col.append(task_col[-1] + len(cl))
    return labels, classes, np.array(task_col)


def fit_tasks(W, Y, variant, alpha=0.2, tol=1e-3, max_iter=1000):
    labels, classes, task_col = encode(Y)
    s, d = degrees(W)
    r = propagate(W, d if variant == SPREADING else s, labels, task_col, variant, alpha, tol, max_iter)
    return finish(r["F"], task_col), r["n_iter"], classes, task_col


def standardize(X):
    """ops.attr_scale: chunks of 256 rows added in order, then the chunk sums; population variance; a constant column becomes 0."""
    X = np.asarray(X, np.float64)
    rows = X.shape[0]

    def total(V):
        acc = np.zeros(V.shape[1])
        for c0 in range(0, rows, 256):
            part = np.zeros(V.shape[1])
            for r in range(c0, min(c0 + 256, rows)):
                part = part + V[r]
            acc = acc + part
        return acc
    mean = total(X) / rows
    std = np.sqrt(total((X - mean) * (X - mean)) / rows)
    return (X - mean) / np.where(std == 0.0, 1.0, std)


def learner_pick(dist, task_col, cand, strategy, taking_part=None):
    sc = scores(dist, task_col, cand)
    row = {"E": "E", "LC": "LC_TASKS", "MS": "MS_TASKS"}[strategy]
    return int(select(sc[SCORES[row]], 1, strategy == "E", taking_part)[0])


def query_and_teach(X_train, Y_train, X_pool, Y_pool, n_queries, variant, gamma, strategy, alpha=0.2, tol=1e-3, max_iter=1000):
    """ActiveLearner.query_and_teach_n_times over the fixed union [train; pool] (the reuse route): -> original pool indices."""
    Xs = standardize(np.vstack([X_train, X_pool]))
    W = rbf_affinity(Xs, gamma)
    n_train = len(X_train)
    Y = np.vstack([Y_train, np.full_like(np.asarray(Y_pool), -1)])
    truth = np.vstack([Y_train, Y_pool])
    labels_all, _, task_col = encode(truth)                     # class columns of the whole loop: every label that can appear
    in_pool = np.ones(len(X_pool), bool)
    cand = n_train + np.arange(len(X_pool))
    s, d = degrees(W)
    picks = []
    for _ in range(n_queries):
        labels = np.where(Y == -1, -1, labels_all)
        r = propagate(W, d if variant == SPREADING else s, labels, task_col, variant, alpha, tol, max_iter)
        p = learner_pick(finish(r["F"], task_col), task_col, cand, strategy, in_pool)
        picks.append(p)
        in_pool[p] = False
        Y[n_train + p] = truth[n_train + p]
    return picks
