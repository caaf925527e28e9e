"""fp64 numpy oracle of the integrated gradients of the compound-protein interaction multitask network
(sample_chem/compound-protein_interaction/multitask.py:35-51 through kgcn visualize).

  literal      the loop of kgcn/visualization.py:187-260 (CompoundVisualizer.cal_integrated_gradients) for ONE compound and ONE task:
               for k in range(D) the inputs named by the modal set are scaled by (k + 1) / D (:195-199; kgcn/feed.py:88-131 scales
               the features and the values of EVERY adjacency channel), the gradient of prediction[:, t, 0] with respect to the
               features and the channel-0 values is taken at that feed (:200-204) and IG[modal] += grad * data / D (:205);
               grad_prod / grad are the single scale-1 step (:206-231); start and end come from the scale-0 and scale-1 feeds
               (:262-286).  The per-step gradients are analytic (grads), checked against central differences by the tests.
  closed_form  the algebra csrc/cpiig.hip and visualization.cpi_integrated_gradients implement: P, Q, Y0 once, the sweep over
               alpha_k P + gamma_k Q, one GraphConv backward per task.
  sweep        what ops.cpi_ig returns for given P, Q, u, e and copy coefficients.

params: {"w": [W_ch [F, Wd]], "b": [b_ch [Wd]], "kernel": V [Wd, 2 T], "bias": c [2 T]}; adjs: dense [N, N] per channel,
A[i, j] the value of entry (row i, column j); a stored entry is a non-zero one.  Task t's prediction is the second entry of the
two-way softmax over (o[t], o[T + t]) (models.CPIMultitaskNet: logits[b, c, t] = out[b, c T + t])."""
import numpy as np


def sigmoid(z):
    z = np.asarray(z, np.float64)
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def dsigmoid(z):
    """sigmoid(z) (1 - sigmoid(z)) without cancellation."""
    e = np.exp(-np.abs(np.asarray(z, np.float64)))
    return e / ((1.0 + e) * (1.0 + e))


def _p64(params):
    return ([np.asarray(w, np.float64) for w in params["w"]], [np.asarray(b, np.float64).reshape(-1) for b in params["b"]],
            np.asarray(params["kernel"], np.float64), np.asarray(params["bias"], np.float64).reshape(-1))


def task_head(params, t):
    """u_t = V[:, T + t] - V[:, t], e_t = c[T + t] - c[t]: softmax(o[t], o[T + t])[1] = sigmoid(h . u_t + e_t)."""
    _, _, V, c = _p64(params)
    T = V.shape[1] // 2
    return V[:, T + t] - V[:, t], c[T + t] - c[t]


def forward(params, x, adjs, t):
    """multitask.py:39-44 for one compound -> (prediction[:, t, 0], Z, H): Z = sum_ch A_ch (x W_ch + 1 b_ch^T) (kgcn/layers.py:64-104),
    H = sigmoid(Z), h = the sum over ALL N rows (GraphGather; a padded row contributes sigmoid(0) = 0.5), o = h V + c."""
    W, b, V, c = _p64(params)
    T = V.shape[1] // 2
    x = np.asarray(x, np.float64)
    Z = sum(np.asarray(A, np.float64) @ (x @ W[ch] + b[ch][None, :]) for ch, A in enumerate(adjs))
    H = sigmoid(Z)
    o = H.sum(0) @ V + c
    m = max(o[t], o[T + t])
    ex = np.exp(np.array([o[t] - m, o[T + t] - m]))
    return float(ex[1] / ex.sum()), Z, H


def grads(params, x, adjs, t):
    """d prediction[:, t, 0] / d (fed features [N, F]) and / d (fed channel-0 adjacency [N, N], every position) at the feed (x, adjs)."""
    W, b, _, _ = _p64(params)
    u, _ = task_head(params, t)
    x = np.asarray(x, np.float64)
    p, Z, _ = forward(params, x, adjs, t)
    dZ = p * (1.0 - p) * u[None, :] * dsigmoid(Z)
    dx = sum(np.asarray(A, np.float64).T @ dZ @ W[ch].T for ch, A in enumerate(adjs))
    dA0 = dZ @ (x @ W[0] + b[0][None, :]).T
    return dx, dA0, p


def modal_targets(modal):
    return ("features", "adjs") if modal == "all" else (modal,)


def literal(params, x, adjs, t, modal="all", method="ig", D=100):
    """kgcn/visualization.py:187-286 for one compound and task -> {"features_IG", "adjs_IG", "start", "end", "sum_of_IG"} (the
    modals of `modal` only).  adjs_IG is dense [N, N] and zero off the stored entries of channel 0 (the gradient is taken with
    respect to the sparse tensor's values)."""
    targets = modal_targets(modal)
    x = np.asarray(x, np.float64)
    adjs = [np.asarray(A, np.float64) for A in adjs]
    stored = adjs[0] != 0

    def feed(scale):                                   # kgcn/feed.py:88-131
        return (x * scale if "features" in targets else x), ([A * scale for A in adjs] if "adjs" in targets else adjs)

    ig = {m: 0.0 for m in targets}
    data = {"features": x, "adjs": adjs[0]}
    if method == "ig":
        steps = [((k + 1) / float(D), 1.0 / D) for k in range(D)]           # :195-205
    elif method in ("grad_prod", "grad"):
        steps = [(1.0, 1.0)]                                                # :206-231
    else:
        raise ValueError(method)
    for scale, weight in steps:
        xs, As = feed(scale)
        dx, dA0, _ = grads(params, xs, As, t)
        g = {"features": dx, "adjs": dA0 * stored}
        for m in targets:
            ig[m] = ig[m] + weight * (g[m] if method == "grad" else g[m] * data[m])
    out = {m + "_IG": ig[m] for m in targets}
    out["start"] = forward(params, *feed(0.0), t)[0]
    out["end"] = forward(params, *feed(1.0), t)[0]
    out["sum_of_IG"] = float(sum(ig[m].sum() for m in targets))
    return out


def copy_coefficients(modal, method, D):
    """The copies of the closed form, derived here independently of the package: scales s_k and weights w_k (k = 0 is the
    start copy of weight 0), a_k = s_k where the features are scaled, c_k = s_k where the adjacency values are."""
    targets = modal_targets(modal)
    if method == "ig":
        s = np.arange(D + 1, dtype=np.float64) / D
        w = np.concatenate([[0.0], np.full(D, 1.0 / D)])
    else:
        s, w = np.array([0.0, 1.0]), np.array([0.0, 1.0])
    a = s if "features" in targets else np.ones_like(s)
    c = s if "adjs" in targets else np.ones_like(s)
    return targets, s, w, a, c


def products(params, x, adjs):
    """P = sum_ch A_ch x W_ch, Q[n, :] = sum_ch rowsum(A_ch)[n] b_ch, Y0 = x W_0."""
    W, b, _, _ = _p64(params)
    x = np.asarray(x, np.float64)
    P = sum(np.asarray(A, np.float64) @ x @ W[ch] for ch, A in enumerate(adjs))
    Q = sum(np.asarray(A, np.float64).sum(1)[:, None] * b[ch][None, :] for ch, A in enumerate(adjs))
    return P, Q, x @ W[0]


def sweep(P, Q, u, e, alpha, gamma, wA, wB=None):
    """ops.cpi_ig for one compound: P, Q [N, Wd], u [T, Wd], e [T], per-copy alpha, gamma, wA, wB [K] ->
    (p [K, T], GA [T, N, Wd], GB or None)."""
    P, Q, u, e = (np.asarray(v, np.float64) for v in (P, Q, u, e))
    K, T = len(alpha), u.shape[0]
    p = np.zeros((K, T))
    GA = np.zeros((T,) + P.shape)
    GB = None if wB is None else np.zeros_like(GA)
    for k in range(K):
        Z = float(alpha[k]) * P + float(gamma[k]) * Q
        d = dsigmoid(Z)
        s = sigmoid(Z).sum(0)
        for t in range(T):
            x = s @ u[t] + e[t]
            p[k, t] = sigmoid(x)
            G = dsigmoid(x) * u[t][None, :] * d
            GA[t] += float(wA[k]) * G
            if wB is not None:
                GB[t] += float(wB[k]) * G
    return p, GA, GB


def closed_form(params, x, adjs, t, modal="all", method="ig", D=100):
    """The same quantities as literal() from P, Q, Y0 and the weighted sums of the sweep."""
    W, b, _, _ = _p64(params)
    targets, s, w, a, c = copy_coefficients(modal, method, D)
    x = np.asarray(x, np.float64)
    adjs = [np.asarray(A, np.float64) for A in adjs]
    P, Q, Y0 = products(params, x, adjs)
    u, e = task_head(params, t)
    p, Gc, _ = sweep(P, Q, u[None, :], [e], a * c, c, w * c)
    _, Ga, _ = sweep(P, Q, u[None, :], [e], a * c, c, w * a)
    _, G1, _ = sweep(P, Q, u[None, :], [e], a * c, c, w)
    raw = method == "grad"
    out = {}
    if "features" in targets:
        g = sum(A.T @ Gc[0] @ W[ch].T for ch, A in enumerate(adjs))
        out["features_IG"] = g if raw else x * g
    if "adjs" in targets:
        g = (Ga[0] @ Y0.T + (G1[0] @ b[0])[:, None]) * (adjs[0] != 0)
        out["adjs_IG"] = g if raw else adjs[0] * g
    out["start"], out["end"] = float(p[0, 0]), float(p[-1, 0])
    out["sum_of_IG"] = float(sum(out[m + "_IG"].sum() for m in targets))
    return out


# ---- test data --------------------------------------------------------------------------------------------------------------
def make_compounds(rng, sizes, N, F, channels=1):
    """Compounds of `sizes` valid nodes padded to N -> (x [G, N, F], dense [channels][G, N, N]).  Directed entries with values in
    {0.5, 1, 2}; a compound of size 0 has no entry at all; node 0 of every other compound holds its self loop only (nobody points
    at it either in channel 0); rows past the size are padding (zero features, no entries)."""
    G = len(sizes)
    x = np.zeros((G, N, F), np.float32)
    dense = [np.zeros((G, N, N), np.float32) for _ in range(channels)]
    for g, m in enumerate(sizes):
        if m == 0:
            continue
        x[g, :m] = rng.standard_normal((m, F)).astype(np.float32)
        for ch in range(channels):
            A = dense[ch][g]
            A[0, 0] = 1.0
            for i in range(1, m):
                A[i, i] = 1.0
                for j in rng.choice(np.arange(1, m), size=min(m - 1, 1 + ch + int(rng.integers(0, 3))), replace=False):
                    if j != i:
                        A[i, j] = float(rng.choice([0.5, 1.0, 2.0]))
    return x, dense


def make_params(rng, F, Wd, T, channels=1, scale=1.0):
    return {"w": [(rng.standard_normal((F, Wd)) * scale / np.sqrt(F)).astype(np.float32) for _ in range(channels)],
            "b": [(rng.standard_normal(Wd) * 0.2 * scale).astype(np.float32) for _ in range(channels)],
            "kernel": (rng.standard_normal((Wd, 2 * T)) / np.sqrt(Wd)).astype(np.float32),
            "bias": (rng.standard_normal(2 * T) * 0.1).astype(np.float32)}
