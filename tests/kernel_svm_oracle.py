"""numpy fp64 oracle of the batched C-SVC solver (csrc/svm.hip through kgcn_amd/ops.py svm_smo_batch / svm_decision_batch /
svm_vote and kgcn_amd.graph_kernel.svm_fit).  Test infrastructure only; it shares no code with the module under test.

It restates libsvm's svm.cpp (the solver scikit-learn's SVC wraps) for C-SVC over a precomputed kernel, without shrinking and
without the kernel cache, in fp64 throughout (libsvm keeps its cached rows Q_i in float32; this solver and the device do not):
  Solver::Solve               the main loop and the clipped two-variable update, both label cases
  Solver::select_working_set  second-order working-set selection (WSS 2 of Fan, Chen, Lin 2005), TAU = 1e-12
  Solver::calculate_rho       the mean of y G over the free vectors, or the midpoint of the bounds
  svm_predict_values          the decision value and the one-vs-one vote
A problem is (idx, sign, C): rows idx of K with labels sign = +-1.  Q_ij = y_i y_j K[idx_i, idx_j]; p = -1; alpha starts at 0,
so G starts at -1.

What is stated so that the device can be compared bit for bit (inside an iteration everything is element-wise numpy, exact
products by +-1 and 2, and exact selections):
  * ties: libsvm scans t = 0, 1, ... with `>=` (i) and `<=` (j), so among equal values the LAST index wins;
  * quad_coef = (QD_i + QD_j) - 2 K_ij for every label pair (libsvm's +-2 y_i Q_ij is that value exactly);
  * the gradient: G_t = G_t + ((Q_it * d_alpha_i) + (Q_jt * d_alpha_j)): two products, their sum, one addition, nothing fused;
  * rho with free vectors: acc = +0.0, acc = acc + y_t G_t over the free t ascending, rho = acc / count;
  * the decision: acc = +0.0, acc = acc + (alpha_t y_t) * K[r, idx_t] for t = 0, 1, ... over ALL training rows, dec = acc - rho."""
import numpy as np

TAU = 1e-12
INF = np.inf


def default_max_iter(n):
    """libsvm's warning threshold (svm.cpp Solver::Solve: max(10000000, l > INT_MAX / 100 ? INT_MAX : 100 * l))."""
    return max(10_000_000, 100 * int(n))


def _last_argmax(v):
    return len(v) - 1 - int(np.argmax(v[::-1]))


def _last_argmin(v):
    return len(v) - 1 - int(np.argmin(v[::-1]))


def smo(K, idx, sign, C, tol=1e-3, max_iter=None):
    """-> dict(alpha [n], G [n], rho, n_iter, converged).  Stops when m(alpha) - M(alpha) < tol or after max_iter updates
    (converged False; alpha, G and rho are then the state after max_iter iterations, as libsvm returns it with a warning)."""
    K = np.asarray(K, np.float64)
    idx = np.asarray(idx, np.int64).reshape(-1)
    y = np.asarray(sign, np.float64).reshape(-1)
    n = idx.shape[0]
    assert n >= 1 and y.shape[0] == n and np.all(np.abs(y) == 1.0)
    C = np.float64(C)
    Ks = K[np.ix_(idx, idx)]
    QD = np.diag(Ks).copy()                                       # svm.cpp SVC_Q: QD[i] = kernel(i, i)
    alpha = np.zeros(n)                                           # svm.cpp solve_c_svc: alpha = 0, minus_ones = -1
    G = -np.ones(n)                                               # Solver::Solve: G = p + Q alpha
    pos = y > 0
    max_iter = default_max_iter(n) if max_iter is None else int(max_iter)
    it, converged = 0, False
    while it < max_iter:
        # ---- select_working_set: i = argmax over I_up of -y_t G_t (`>=`: the last index among equals)
        up = np.where(pos, alpha < C, alpha > 0.0)                # y=+1: !is_upper_bound; y=-1: !is_lower_bound
        if not up.any():
            converged = True                                      # Gmax = -INF: no j has grad_diff > 0, the function returns 1
            break
        yG = y * G
        i = _last_argmax(np.where(up, -yG, -INF))
        Gmax = -yG[i]
        Ki = Ks[i]
        # ---- j = argmin over I_low with grad_diff > 0 of -grad_diff^2 / quad_coef (`<=`: the last index among equals)
        low = np.where(pos, alpha > 0.0, alpha < C)               # y=+1: !is_lower_bound; y=-1: !is_upper_bound
        Gmax2 = np.max(np.where(low, yG, -INF))
        grad_diff = Gmax + yG
        quad = (QD[i] + QD) - 2.0 * Ki
        quad = np.where(quad > 0.0, quad, TAU)
        obj = -(grad_diff * grad_diff) / quad
        cand = low & (grad_diff > 0.0)
        if Gmax + Gmax2 < tol or not cand.any():
            converged = True
            break
        j = _last_argmin(np.where(cand, obj, INF))
        it += 1
        # ---- Solver::Solve: update alpha[i] and alpha[j], handle bounds carefully
        Kj = Ks[j]
        quad = (QD[i] + QD[j]) - 2.0 * Ki[j]
        if quad <= 0.0:
            quad = TAU
        ai, aj = alpha[i], alpha[j]
        if y[i] != y[j]:
            delta = (-G[i] - G[j]) / quad
            diff = ai - aj
            ai, aj = ai + delta, aj + delta
            if diff > 0.0:
                if aj < 0.0:
                    aj, ai = 0.0, diff
            else:
                if ai < 0.0:
                    ai, aj = 0.0, -diff
            if diff > C - C:                                      # C_i - C_j: one C for both classes
                if ai > C:
                    ai, aj = C, C - diff
            else:
                if aj > C:
                    aj, ai = C, C + diff
        else:
            delta = (G[i] - G[j]) / quad
            tot = ai + aj
            ai, aj = ai - delta, aj + delta
            if tot > C:
                if ai > C:
                    ai, aj = C, tot - C
            else:
                if aj < 0.0:
                    aj, ai = 0.0, tot
            if tot > C:
                if aj > C:
                    aj, ai = C, tot - C
            else:
                if ai < 0.0:
                    ai, aj = 0.0, tot
        dai, daj = np.float64(ai) - alpha[i], np.float64(aj) - alpha[j]
        alpha[i], alpha[j] = ai, aj
        # ---- update G: G[k] += Q_i[k] * delta_alpha_i + Q_j[k] * delta_alpha_j
        G = G + (((y[i] * y) * Ki) * dai + ((y[j] * y) * Kj) * daj)
    return {"alpha": alpha, "G": G, "rho": rho(alpha, G, y, C), "n_iter": it, "converged": converged}


def rho(alpha, G, y, C):
    """Solver::calculate_rho."""
    yG = y * G
    upper, lower = alpha >= C, alpha <= 0.0
    free = ~upper & ~lower
    if free.any():
        acc = np.cumsum(np.concatenate([[0.0], yG[free]]))[-1]    # sequential, from +0.0
        return float(acc / np.float64(int(free.sum())))
    ub_set = (upper & (y < 0)) | (lower & ~upper & (y > 0))
    lb_set = (upper & (y > 0)) | (lower & ~upper & (y < 0))
    ub = np.min(np.where(ub_set, yG, INF))
    lb = np.max(np.where(lb_set, yG, -INF))
    return float((ub + lb) / 2.0)


def decision(K, idx, sign, alpha, rho_value, rows):
    """libsvm's dec_value of every row: sum_t (alpha_t y_t) K[r, idx_t] - rho, t ascending over all training rows.  Positive:
    the +1 class.  (scikit-learn's two-class decision_function is its negative.)"""
    K = np.asarray(K, np.float64)
    idx = np.asarray(idx, np.int64).reshape(-1)
    rows = np.asarray(rows, np.int64).reshape(-1)
    coef = np.asarray(alpha, np.float64) * np.asarray(sign, np.float64)
    acc = np.zeros(rows.shape[0])
    for t in range(idx.shape[0]):
        acc = acc + coef[t] * K[rows, idx[t]]
    return acc - np.float64(rho_value)


def pairs(k):
    """libsvm's order of the one-vs-one problems: (0, 1), (0, 2), ..., (1, 2), ...; the first class of a pair is its +1."""
    return [(a, b) for a in range(k) for b in range(a + 1, k)]


def vote(dec, k):
    """svm_predict_values: dec [pairs, rows] -> class index [rows]; dec > 0 votes for the pair's first class, else for its
    second; the class with the most votes, the lowest index among equals."""
    dec = np.asarray(dec, np.float64).reshape(len(pairs(k)), -1)
    votes = np.zeros((k, dec.shape[1]), np.int64)
    for p, (a, b) in enumerate(pairs(k)):
        votes[a] += dec[p] > 0
        votes[b] += ~(dec[p] > 0)
    return np.argmax(votes, axis=0).astype(np.int32)              # np.argmax: the first maximum


def ovo_problems(y_codes, train):
    """The pair problems of one training set -> [(a, b, idx, sign)]: the rows of classes a and b in the order of `train`,
    +1 for a.  (libsvm groups the rows by class first; the order inside a problem only permutes the sums.)"""
    train = np.asarray(train, np.int64)
    codes = np.asarray(y_codes)[train]
    k = int(np.max(y_codes)) + 1
    out = []
    for a, b in pairs(k):
        keep = (codes == a) | (codes == b)
        out.append((a, b, train[keep], np.where(codes[keep] == a, 1, -1).astype(np.int8)))
    return out


def nested_folds(n, test_splits=5, val_splits=5):
    """KFold(n_splits) without shuffling, nested as kgcn_amd.graph_kernel.svm_cv nests it -> [(train, val, test)] index arrays,
    outer split major."""
    def kfold(m, splits):
        sizes = np.full(splits, m // splits, np.int64)
        sizes[:m % splits] += 1
        stops = np.cumsum(sizes)
        return [(np.r_[0:s - z, s:m], np.arange(s - z, s)) for s, z in zip(stops, sizes)]
    out = []
    for tv_pos, te in kfold(n, test_splits):
        for a, b in kfold(len(tv_pos), val_splits):
            out.append((tv_pos[a], tv_pos[b], te))
    return out
