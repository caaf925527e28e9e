"""numpy fp64 statement of the vector-modality models and the regression head (kgcn_amd.ops.dense_bn, masked_squared_error,
regression_metrics; models.MultimodalVecGCN, models.MultimodalRegressionGCN), with hand-written gradients that
tests/test_vecmodal_oracle.py checks against central differences.  Adjacency is dense [B, N, N] here (a dummy graph is all zero);
BatchNormalization runs in learning phase 0: the moving statistics are constants."""
import numpy as np

F64 = np.float64


def act_fwd(z, act):
    if act in (None, "none"):
        return z
    if act == "relu":
        return np.maximum(z, 0.0)
    if act == "tanh":
        return np.tanh(z)
    if act == "sigmoid":
        return 1.0 / (1.0 + np.exp(-z))
    raise ValueError(act)


def act_grad(y, act):
    """derivative in terms of the activation's output"""
    if act in (None, "none"):
        return np.ones_like(y)
    if act == "relu":
        return (y > 0).astype(F64)
    if act == "tanh":
        return 1.0 - y * y
    if act == "sigmoid":
        return y * (1.0 - y)
    raise ValueError(act)


# ---- Dense + BN (learning phase 0) + activation ------------------------------------------------------------------------------------
def dense_bn_fwd(x, p, act=None, eps=1e-3):
    """p: {"w", "b"} and, with batch normalisation, {"gamma", "beta", "mean", "var"} -> y [B, N]."""
    x = np.asarray(x, F64)
    pre = x @ np.asarray(p["w"], F64) + np.asarray(p["b"], F64)
    if "gamma" in p:
        s = np.asarray(p["gamma"], F64) / np.sqrt(np.asarray(p["var"], F64) + eps)
        pre = s * (pre - np.asarray(p["mean"], F64)) + np.asarray(p["beta"], F64)
    return act_fwd(pre, act)


def dense_bn_bwd(x, p, dy, act=None, eps=1e-3):
    """-> {"x", "w", "b"[, "gamma", "beta"]}: the gradients of sum(dy * y)."""
    x, w = np.asarray(x, F64), np.asarray(p["w"], F64)
    pre = x @ w + np.asarray(p["b"], F64)
    y = dense_bn_fwd(x, p, act, eps)
    dz = np.asarray(dy, F64) * act_grad(y, act)
    g = {}
    if "gamma" in p:
        rstd = 1.0 / np.sqrt(np.asarray(p["var"], F64) + eps)
        g["gamma"] = (dz * (pre - np.asarray(p["mean"], F64)) * rstd).sum(axis=0)
        g["beta"] = dz.sum(axis=0)
        dz = dz * (np.asarray(p["gamma"], F64) * rstd)
    g["x"], g["w"], g["b"] = dz @ w.T, x.T @ dz, dz.sum(axis=0)
    return g


# ---- losses -------------------------------------------------------------------------------------------------------------------------
def masked_softmax_ce(logits, labels, mask):
    """model_multimodal_vec.py:112-120 -> (cost_opt, cost_sum, d cost_opt / d logits)."""
    z = np.asarray(logits, F64)
    labels, mask = np.asarray(labels, F64), np.asarray(mask, F64).reshape(-1)
    zs = z - z.max(axis=1, keepdims=True)
    logp = zs - np.log(np.exp(zs).sum(axis=1, keepdims=True))
    cost = mask * -(labels * logp).sum(axis=1)
    d = mask[:, None] * (np.exp(logp) * labels.sum(axis=1, keepdims=True) - labels)
    return cost.mean(), cost.sum(), d / z.shape[0]


def masked_squared_error(pred, labels, mask_label):
    """model_multimodal_regression.py:94-101 -> dict(cost_opt, cost_sum, error_sum [T], count [T], dpred = d cost_sum / d pred)."""
    p, y, m = (np.asarray(v, F64) for v in (pred, labels, mask_label))
    loss = m * (y - p) ** 2
    return {"cost_opt": loss.mean(), "cost_sum": loss.sum(), "error_sum": loss.sum(axis=0), "count": m.sum(axis=0),
            "dpred": -2.0 * m * (y - p)}


def regression_sums(pred, label, mask=None):
    """ops.regression_metrics -> [T, 6]: n, sum y, sum (y - mean)^2, sum (y - p)^2, sum log(y / p) over positive finite ratios,
    the count of the other rows."""
    p, y = np.asarray(pred, F64), np.asarray(label, F64)
    out = np.zeros((p.shape[1], 6), F64)
    for t in range(p.shape[1]):
        sel = np.ones(p.shape[0], bool) if mask is None else np.asarray(mask)[:, t] != 0
        yt, pt = y[sel, t], p[sel, t]
        with np.errstate(all="ignore"):
            q = yt / pt
        ok = (q > 0) & np.isfinite(q)
        mean = yt.mean() if yt.size else 0.0
        out[t] = [yt.size, yt.sum(), ((yt - mean) ** 2).sum(), ((yt - pt) ** 2).sum(), np.log(q[ok]).sum(), (~ok).sum()]
    return out


# ---- graph layers on dense adjacency --------------------------------------------------------------------------------------------------
def _graph_bn(x, p, sizes, act, eps=1e-3):
    """GraphBatchNormalization in learning phase 0 over the valid rows, zeros on the padding rows, then the activation."""
    B, N, _ = x.shape
    valid = (np.arange(N)[None, :] < np.asarray(sizes).reshape(B, 1))[:, :, None]
    s = np.asarray(p["gamma"], F64) / np.sqrt(np.asarray(p["var"], F64) + eps)
    z = np.where(valid, s * (x - np.asarray(p["mean"], F64)) + np.asarray(p["beta"], F64), 0.0)
    return act_fwd(z, act), valid


def _graph_bn_bwd(x, p, sizes, act, dy, eps=1e-3):
    y, valid = _graph_bn(x, p, sizes, act, eps)
    dz = np.where(valid, dy * act_grad(y, act), 0.0)
    rstd = 1.0 / np.sqrt(np.asarray(p["var"], F64) + eps)
    g = {"gamma": (dz * (x - np.asarray(p["mean"], F64)) * rstd).sum(axis=(0, 1)), "beta": dz.sum(axis=(0, 1))}
    return dz * np.asarray(p["gamma"], F64) * rstd, g


# ---- models.MultimodalVecGCN ------------------------------------------------------------------------------------------------------------
def vec_model(features, adj, vectors, P, labels=None, mask=None):
    """P: {"conv": {w, b}, "dense": {w, b}, "tower": [3 x dense_bn dict], "hidden": dense_bn dict, "out": {w, b}} ->
    (logits, loss tuple or None, gradients in P's structure or None)."""
    x, A, v = np.asarray(features, F64), np.asarray(adj, F64), np.asarray(vectors, F64)
    xw = x @ np.asarray(P["conv"]["w"], F64) + np.asarray(P["conv"]["b"], F64)
    h1 = act_fwd(A @ xw, "sigmoid")                                               # GraphConv(50) sigmoid
    h2 = act_fwd(h1 @ np.asarray(P["dense"]["w"], F64) + np.asarray(P["dense"]["b"], F64), "sigmoid")
    graph = h2.sum(axis=1)                                                        # GraphGather: every node row, padding included
    t = [v]
    for p in P["tower"]:
        t.append(dense_bn_fwd(t[-1], p, "relu"))
    joined = np.concatenate([t[-1], graph], axis=1)
    hid = dense_bn_fwd(joined, P["hidden"], "relu")
    logits = dense_bn_fwd(hid, P["out"], None)
    if labels is None:
        return logits, None, None
    cost_opt, cost_sum, dlog = masked_softmax_ce(logits, labels, mask)
    G = {"tower": [None] * len(P["tower"])}
    g = dense_bn_bwd(hid, P["out"], dlog, None)
    G["out"] = g
    g = dense_bn_bwd(joined, P["hidden"], g["x"], "relu")
    G["hidden"] = g
    vw = t[-1].shape[1]
    dvec, dgraph = g["x"][:, :vw], g["x"][:, vw:]
    for i in reversed(range(len(P["tower"]))):
        g = dense_bn_bwd(t[i], P["tower"][i], dvec, "relu")
        G["tower"][i] = g
        dvec = g["x"]
    dh2 = np.broadcast_to(dgraph[:, None, :], h2.shape) * act_grad(h2, "sigmoid")
    G["dense"] = {"w": np.einsum("bnd,bne->de", h1, dh2), "b": dh2.sum(axis=(0, 1))}
    dh1 = (dh2 @ np.asarray(P["dense"]["w"], F64).T) * act_grad(h1, "sigmoid")
    dxw = np.swapaxes(A, 1, 2) @ dh1
    G["conv"] = {"w": np.einsum("bnf,bnd->fd", x, dxw), "b": dxw.sum(axis=(0, 1))}
    return logits, (cost_opt, cost_sum), G


# ---- models.MultimodalRegressionGCN -----------------------------------------------------------------------------------------------------
def regression_model(features, sizes, vectors, P, labels=None, mask_label=None):
    """P: {"gd": [3 x {w, b}], "bn": [3 x {gamma, beta, mean, var}], "vec": dense_bn dict, "out": {w, b}} ->
    (predictions, masked_squared_error dict or None, gradients of cost_opt in P's structure or None)."""
    x, v = np.asarray(features, F64), np.asarray(vectors, F64)
    acts = ("relu", "relu", None)
    ins, pres = [x], []
    for i in range(3):
        pre = ins[-1] @ np.asarray(P["gd"][i]["w"], F64) + np.asarray(P["gd"][i]["b"], F64)
        pres.append(pre)
        ins.append(_graph_bn(pre, P["bn"][i], sizes, acts[i])[0])
    graph = np.tanh(ins[-1].sum(axis=1))
    vec = dense_bn_fwd(v, P["vec"], "relu")
    joined = np.concatenate([vec, graph], axis=1)
    pred = dense_bn_fwd(joined, P["out"], None)
    if labels is None:
        return pred, None, None
    L = masked_squared_error(pred, labels, mask_label)
    G = {"gd": [None] * 3, "bn": [None] * 3}
    g = dense_bn_bwd(joined, P["out"], L["dpred"] / pred.size, None)
    G["out"] = g
    vw = vec.shape[1]
    G["vec"] = dense_bn_bwd(v, P["vec"], g["x"][:, :vw], "relu")
    dgraph = g["x"][:, vw:] * (1.0 - graph * graph)
    d = np.broadcast_to(dgraph[:, None, :], ins[-1].shape)
    for i in reversed(range(3)):
        dpre, G["bn"][i] = _graph_bn_bwd(pres[i], P["bn"][i], sizes, acts[i], d)
        G["gd"][i] = {"w": np.einsum("bnf,bnd->fd", ins[i], dpre), "b": dpre.sum(axis=(0, 1))}
        d = dpre @ np.asarray(P["gd"][i]["w"], F64).T
    return pred, L, G


# ---- helpers of the tests -------------------------------------------------------------------------------------------------------------
def draw_dense_bn(rng, k, n, batch_norm=True, trivial_stats=False):
    lim = np.sqrt(6.0 / (k + n))
    p = {"w": rng.uniform(-lim, lim, (k, n)), "b": 0.1 * rng.standard_normal(n)}
    if batch_norm:
        p.update(gamma=1.0 + 0.2 * rng.standard_normal(n), beta=0.1 * rng.standard_normal(n),
                 mean=np.zeros(n) if trivial_stats else 0.3 * rng.standard_normal(n),
                 var=np.ones(n) if trivial_stats else 0.5 + rng.random(n))
    return {k_: np.asarray(v, np.float32) for k_, v in p.items()}


def draw_vec_model(rng, feature_dim, vec_dim, label_dim=2):
    widths = (vec_dim, 300, 100, 64)
    lim = np.sqrt(6.0 / (feature_dim + 50))
    f32 = lambda a: np.asarray(a, np.float32)
    return {"conv": {"w": f32(rng.uniform(-lim, lim, (feature_dim, 50))), "b": f32(0.1 * rng.standard_normal(50))},
            "dense": {"w": f32(rng.uniform(-0.24, 0.24, (50, 50))), "b": f32(0.1 * rng.standard_normal(50))},
            "tower": [draw_dense_bn(rng, widths[i], widths[i + 1]) for i in range(3)],
            "hidden": draw_dense_bn(rng, 114, 52), "out": draw_dense_bn(rng, 52, label_dim, batch_norm=False)}


def draw_regression_model(rng, feature_dim, vec_dim, label_dim=2):
    dims = (feature_dim, 32, 32, 32)
    P = {"gd": [], "bn": []}
    for i in range(3):
        q = draw_dense_bn(rng, dims[i], dims[i + 1])
        P["gd"].append({"w": q["w"], "b": q["b"]})
        P["bn"].append({k: q[k] for k in ("gamma", "beta", "mean", "var")})
    P["vec"] = draw_dense_bn(rng, vec_dim, 8)
    P["out"] = draw_dense_bn(rng, 40, label_dim, batch_norm=False)
    return P


TRAINABLE = ("w", "b", "gamma", "beta")


def flatten(tree, keys=TRAINABLE, prefix=""):
    """-> [(path, array)] of the trainable leaves of a parameter / gradient tree, in a fixed order."""
    out = []
    if isinstance(tree, dict):
        for k in sorted(tree):
            if isinstance(tree[k], (dict, list)):
                out += flatten(tree[k], keys, prefix + k + ".")
            elif k in keys:
                out.append((prefix + k, tree[k]))
    else:
        for i, v in enumerate(tree):
            out += flatten(v, keys, prefix + "%d." % i)
    return out
