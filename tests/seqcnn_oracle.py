"""NumPy fp64 restatement of the protein-sequence CNN, sample_protein/sequence/cnn.py:36-90, and of its building block, Keras
Conv1D(F, k, padding='same', activation) -> MaxPooling1D(pool):

  cnn.py:37     Embedding(S, E)                       rows = table[tokens]
  cnn.py:46-58  3 x [Conv1D(relu, same), MaxPooling1D] conv1d_pool_fwd / conv1d_pool_bwd (dense x [B, L, Cin], or tokens + table)
  cnn.py:60-62  Conv1D(1, 2, same, tanh), squeeze     pool = 1, then [B, T3, 1] -> [B, T3]
  cnn.py:74-77  BatchNormalization, Dense(52), BatchNormalization, relu    keras_bn: learning phase 0 with the initial moving
                                                      statistics, y = gamma x / sqrt(1 + 1e-3) + beta
  cnn.py:79     Dense(label_dim)
  cnn.py:84-90  cost = softmax CE; cost_opt = reduce_mean(cost * labels * class_weight); cost_sum = reduce_sum(cost)

Padding is tests/multimodal_oracle.same_padding's rule; the arg-max of a window is the lowest index among equal maxima
(np.argmax).  conv1d_pool_loop is a plain loop transcription used only to check the vectorised functions.
"""
import numpy as np

F64 = np.float64
BN_EPS = 1e-3


def same_padding(k):
    """TF SAME padding of a stride-1 window of size k: (left, right) -- as tests/multimodal_oracle.same_padding."""
    left = (k - 1) // 2
    return left, k - 1 - left


def act_fwd(z, act):
    if act == "relu":
        return np.maximum(z, 0.0)
    if act == "tanh":
        return np.tanh(z)
    if act in (None, "none"):
        return z
    raise ValueError(act)


def act_dout(a, act):
    """Derivative as a function of the activation's OUTPUT."""
    if act == "relu":
        return (a > 0).astype(F64)
    if act == "tanh":
        return 1.0 - a * a
    return np.ones_like(a)


def conv_rows(x=None, tokens=None, table=None):
    """The conv operand rows [B, L, Cin]: x, or table[tokens] (cnn.py:37)."""
    if tokens is not None:
        return np.asarray(table, F64)[np.asarray(tokens)]
    return np.asarray(x, F64)


def conv1d_pool_fwd(w, b, pool, act, x=None, tokens=None, table=None):
    """-> dict(out [B, L // pool, F], arg [B, T, F], pre [B, L, F] pre-activations, xp the padded rows)."""
    rows = conv_rows(x, tokens, table)
    w, b = np.asarray(w, F64), np.asarray(b, F64)
    B, L, _ = rows.shape
    k, _, F = w.shape
    left, _ = same_padding(k)
    xp = np.zeros((B, L + k - 1, rows.shape[2]), F64)
    xp[:, left:left + L] = rows
    pre = np.broadcast_to(b, (B, L, F)).copy()
    for dk in range(k):
        pre += xp[:, dk:dk + L] @ w[dk]
    T = L // pool
    y = act_fwd(pre[:, :T * pool], act).reshape(B, T, pool, F)
    return dict(out=y.max(axis=2), arg=y.argmax(axis=2), pre=pre, xp=xp, rows=rows, w=w, pool=pool, act=act, tokens=tokens,
                table_shape=None if table is None else np.asarray(table).shape)


def conv1d_pool_bwd(c, g):
    """cache of conv1d_pool_fwd, d out [B, T, F] -> dict(dx [B, L, Cin], dw, db, and dtable in token mode)."""
    w, pool, pre, xp = c["w"], c["pool"], c["pre"], c["xp"]
    B, L, F = pre.shape
    k = w.shape[0]
    T = L // pool
    left, _ = same_padding(k)
    routed = np.zeros((B, T, pool, F), F64)
    bi, ti, fi = np.meshgrid(np.arange(B), np.arange(T), np.arange(F), indexing="ij")
    routed[bi, ti, c["arg"], fi] = np.asarray(g, F64) * act_dout(c["out"], c["act"])
    dpre = np.zeros((B, L, F), F64)
    dpre[:, :T * pool] = routed.reshape(B, T * pool, F)
    dxp = np.zeros_like(xp)
    for dk in range(k):
        dxp[:, dk:dk + L] += dpre @ w[dk].T
    res = dict(dx=dxp[:, left:left + L], db=dpre.sum(axis=(0, 1)),
               dw=np.stack([np.einsum("blc,blf->cf", xp[:, dk:dk + L], dpre) for dk in range(k)]))
    if c["tokens"] is not None:
        res["dtable"] = embedding_grad(c["tokens"], res["dx"], c["table_shape"][0])
    return res


def embedding_grad(tokens, dembedded, symbols):
    dtable = np.zeros((symbols, dembedded.shape[2]), F64)
    np.add.at(dtable, np.asarray(tokens).reshape(-1), np.asarray(dembedded, F64).reshape(-1, dembedded.shape[2]))
    return dtable


def conv1d_pool_loop(w, b, pool, act, x=None, tokens=None, table=None):
    """Literal loop transcription (one output at a time), for small cases -> (out, arg)."""
    rows = conv_rows(x, tokens, table)
    w, b = np.asarray(w, F64), np.asarray(b, F64)
    B, L, Cin = rows.shape
    k, _, F = w.shape
    left = (k - 1) // 2
    T = L // pool
    out, arg = np.zeros((B, T, F), F64), np.zeros((B, T, F), np.int64)
    for bb in range(B):
        for t in range(T):
            for f in range(F):
                best = None
                for j in range(pool):
                    s = b[f]
                    for dk in range(k):
                        l = t * pool + j + dk - left
                        if 0 <= l < L:
                            for ci in range(Cin):
                                s += rows[bb, l, ci] * w[dk, ci, f]
                    v = float(act_fwd(np.float64(s), act))
                    if best is None or v > best:
                        best, arg[bb, t, f] = v, j
                out[bb, t, f] = best
    return out, arg


def window_margins(c):
    """The two conditioning figures of a forward cache: the smallest |pre-activation| (relu layers; inf otherwise) and the
    smallest gap between the two largest DISTINCT candidates of a window (inf where a window has one distinct value)."""
    pool, pre, act = c["pool"], c["pre"], c["act"]
    B, L, F = pre.shape
    T = L // pool
    near_zero = float(np.abs(pre[:, :T * pool]).min()) if (act == "relu" and T > 0) else np.inf
    gap = np.inf
    if pool > 1 and T > 0:
        y = np.sort(act_fwd(pre[:, :T * pool], act).reshape(B, T, pool, F), axis=2)
        d = y[:, :, -1:, :] - y[:, :, :-1, :]
        d = np.where(d > 0, d, np.inf)
        gap = float(d.min())
    return near_zero, gap


# ---- the model ---------------------------------------------------------------------------------------------------------------
def keras_bn(x, gamma, beta):
    """cnn.py:74, :76 under learning phase 0 with moving mean 0 / variance 1."""
    return np.asarray(gamma, F64) * np.asarray(x, F64) / np.sqrt(1.0 + BN_EPS) + np.asarray(beta, F64)


def log_softmax(z):
    m = z.max(axis=1, keepdims=True)
    return z - m - np.log(np.exp(z - m).sum(axis=1, keepdims=True))


def loss(logits, labels, class_weight, mask=None):
    """-> (cost_opt, cost_sum, cost [B]): cost_opt = (1 / (B C)) sum_b mask_b cost_b class_weight[label_b], cost_sum = sum_b
    mask_b cost_b (cnn.py:84-90 at B = 1, extended to any B)."""
    logits, labels = np.asarray(logits, F64), np.asarray(labels, F64)
    B, C = labels.shape
    mask = np.ones(B) if mask is None else np.asarray(mask, F64)
    cost = -(labels * log_softmax(logits)).sum(axis=1)
    wrow = (labels * np.asarray(class_weight, F64)).sum(axis=1)
    return float((mask * cost * wrow).sum() / (B * C)), float((mask * cost).sum()), cost


def loss_reference_literal(logits, labels, class_weight):
    """cnn.py:84-87, :90 evaluated literally (NumPy broadcasting is TF's): defined for B = 1."""
    logits, labels = np.asarray(logits, F64), np.asarray(labels, F64)
    cost = -(labels * log_softmax(logits)).sum(axis=1)               # :84  [B]
    w = labels * np.asarray(class_weight, F64)                        # :85  [B, C]
    return float(np.mean(cost * w)), float(np.sum(cost))              # :87, :90


PARAMS = ("embeddings", "w1", "b1", "w2", "b2", "w3", "b3", "w4", "b4", "gamma1", "beta1", "wh", "bh", "gamma2", "beta2", "wo", "bo")
KERNELS = (4, 3, 2)


def init_params(rng, S, E, L, label_dim=2, widths=(505, 200, 100), hidden=52, scale=1.0):
    """Random parameters of the model's shapes (biases, gamma and beta away from their trivial initial values)."""
    p = {"embeddings": rng.uniform(-1, 1, (S, E)) * scale}
    cin, T = E, L
    for i, (f, k) in enumerate(zip(widths, KERNELS), 1):
        lim = np.sqrt(6.0 / (k * cin + k * f)) * 2
        p["w%d" % i], p["b%d" % i] = rng.uniform(-lim, lim, (k, cin, f)), rng.uniform(-0.1, 0.1, f)
        cin, T = f, T // k
    # the closing tanh layer has ONE filter: glorot limits (fans 2 cin, 2) would give pre-activations several units wide and a
    # saturated tanh everywhere; U(-1, 1) / sqrt(2 cin) keeps them at about 0.6 of the input's rms
    p["w4"], p["b4"] = rng.uniform(-1, 1, (2, cin, 1)) / np.sqrt(2 * cin), rng.uniform(-0.1, 0.1, 1)
    p["gamma1"], p["beta1"] = rng.uniform(0.5, 1.5, T), rng.uniform(-0.2, 0.2, T)
    p["wh"], p["bh"] = rng.uniform(-0.5, 0.5, (T, hidden)), rng.uniform(-0.1, 0.1, hidden)
    p["gamma2"], p["beta2"] = rng.uniform(0.5, 1.5, hidden), rng.uniform(-0.2, 0.2, hidden)
    p["wo"], p["bo"] = rng.uniform(-0.5, 0.5, (hidden, label_dim)), rng.uniform(-0.1, 0.1, label_dim)
    return {k: np.asarray(v, np.float32) for k, v in p.items()}


def model_fwd(p, labels, class_weight, mask=None, tokens=None, embedded=None):
    """cnn.py:36-90 -> cache with logits, cost_opt, cost_sum."""
    p = {k: np.asarray(v, F64) for k, v in p.items()}
    if embedded is not None:
        c1 = conv1d_pool_fwd(p["w1"], p["b1"], 4, "relu", x=embedded)                            # :39-40, :46-48
    else:
        c1 = conv1d_pool_fwd(p["w1"], p["b1"], 4, "relu", tokens=tokens, table=p["embeddings"])  # :37, :46-48
    c2 = conv1d_pool_fwd(p["w2"], p["b2"], 3, "relu", x=c1["out"])                               # :51-53
    c3 = conv1d_pool_fwd(p["w3"], p["b3"], 2, "relu", x=c2["out"])                               # :56-58
    c4 = conv1d_pool_fwd(p["w4"], p["b4"], 1, "tanh", x=c3["out"])                               # :60-61
    s = c4["out"][:, :, 0]                                                                       # :62-66
    n1 = keras_bn(s, p["gamma1"], p["beta1"])                                                    # :74
    h = n1 @ p["wh"] + p["bh"]                                                                   # :75
    n2 = keras_bn(h, p["gamma2"], p["beta2"])                                                    # :76
    r = np.maximum(n2, 0.0)                                                                      # :77
    logits = r @ p["wo"] + p["bo"]                                                               # :79
    cost_opt, cost_sum, _ = loss(logits, labels, class_weight, mask)
    return dict(p=p, convs=(c1, c2, c3, c4), s=s, n1=n1, h=h, n2=n2, r=r, logits=logits, labels=np.asarray(labels, F64),
                class_weight=np.asarray(class_weight, F64), mask=mask, cost_opt=cost_opt, cost_sum=cost_sum)


def model_bwd(c, g_opt=1.0, g_sum=0.0):
    """Gradients of g_opt cost_opt + g_sum cost_sum -> dict over PARAMS (embeddings only in token mode) plus d_embedded (the
    gradient with respect to the first layer's input rows)."""
    p, labels = c["p"], c["labels"]
    B, C = labels.shape
    mask = np.ones(B) if c["mask"] is None else np.asarray(c["mask"], F64)
    wrow = (labels * c["class_weight"]).sum(axis=1)
    sm = np.exp(log_softmax(c["logits"]))
    dce = sm * labels.sum(axis=1, keepdims=True) - labels
    dlog = dce * (mask * (g_sum + g_opt * wrow / (B * C)))[:, None]
    g = {"wo": c["r"].T @ dlog, "bo": dlog.sum(axis=0)}
    dn2 = (dlog @ p["wo"].T) * (c["n2"] > 0)
    s1 = 1.0 / np.sqrt(1.0 + BN_EPS)
    g["gamma2"], g["beta2"] = (dn2 * c["h"]).sum(axis=0) * s1, dn2.sum(axis=0)
    dh = dn2 * p["gamma2"] * s1
    g["wh"], g["bh"] = c["n1"].T @ dh, dh.sum(axis=0)
    dn1 = dh @ p["wh"].T
    g["gamma1"], g["beta1"] = (dn1 * c["s"]).sum(axis=0) * s1, dn1.sum(axis=0)
    d = (dn1 * p["gamma1"] * s1)[:, :, None]
    for i in (4, 3, 2, 1):
        r = conv1d_pool_bwd(c["convs"][i - 1], d)
        g["w%d" % i], g["b%d" % i] = r["dw"], r["db"]
        d = r["dx"]
    g["d_embedded"] = d
    if "dtable" in r:
        g["embeddings"] = r["dtable"]
    return g
