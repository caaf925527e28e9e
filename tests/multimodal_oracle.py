"""fp64 numpy restatement of example_model/model_multimodal.py (the multimodal graph + sequence model of
example_config/multimodal.json), TF 1.15 Keras semantics:

  graph branch  :60-66   GraphConv(50, C) -> sigmoid -> GraphDense(50) -> sigmoid -> GraphGather (sum over all node rows)
  sequence      :73-75   Embedding(S, E), no mask_zero (symbol 0 is a trained row)
                :79-81   Conv1D(50, 4, padding='same', relu): SAME at stride 1 pads (k-1)//2 left, the rest right
                :82      MaxPooling1D(4): stride 4, valid, T' = L // 4; the gradient goes to the lowest index among equal maxima
                :85-87   LSTM(32, return_sequences=False, go_backwards=True): Keras v1 cell, gates i, f, c, o, recurrent
                         activation hard_sigmoid = clip(0.2 x + 0.5, 0, 1) (tf.clip_by_value: the gradient passes at the edges),
                         tanh, zero state, no masking: steps T'-1 .. 0, the output is h after input step 0
  shared        :96-104  concat([sequence 32, graph 50]) -> Dense(52) -> relu -> Dense(label_dim)
  cost          :107-113 mask * softmax_cross_entropy; cost_opt = reduce_mean over the padded batch, cost_sum = reduce_sum

Every function computes in float64 whatever it is given.  The conv-pool and LSTM functions take dtype=np.float32 to evaluate the
same expressions in fp32 instead: that evaluation's distance from the fp64 one is what an honest fp32 implementation costs at
a shape, and the GPU shape sweep (tests/test_gpu_seq_shapes.py) derives its bounds from it."""
import numpy as np

F64 = np.float64


# ---- activations --------------------------------------------------------------------------------------------------------
def hard_sigmoid(z, dtype=F64):
    return np.clip(dtype(0.2) * np.asarray(z, dtype) + dtype(0.5), dtype(0.0), dtype(1.0))


def hard_sigmoid_grad(z, dtype=F64):
    y = dtype(0.2) * np.asarray(z, dtype) + dtype(0.5)
    return np.where((y >= 0.0) & (y <= 1.0), dtype(0.2), dtype(0.0))


def sigmoid(z, dtype=F64):
    return dtype(1.0) / (dtype(1.0) + np.exp(-np.asarray(z, dtype)))


def _rec(act, dtype=F64):
    if act == "hard_sigmoid":
        return (lambda z: hard_sigmoid(z, dtype)), (lambda z, a: hard_sigmoid_grad(z, dtype))
    if act == "sigmoid":
        return (lambda z: sigmoid(z, dtype)), (lambda z, a: a * (dtype(1.0) - a))
    raise ValueError(act)


# ---- embedding + Conv1D(same, relu) + MaxPooling1D ----------------------------------------------------------------------
def same_padding(k):
    """TF SAME padding of a stride-1 window of size k: (left, right)."""
    left = (k - 1) // 2
    return left, k - 1 - left


def conv_same(tokens, table, w, b, dtype=F64):
    """-> (padded embedding [B, L + k - 1, E], conv pre-activation [B, L, F])."""
    tokens = np.asarray(tokens)
    table, w, b = np.asarray(table, dtype), np.asarray(w, dtype), np.asarray(b, dtype)
    B, L = tokens.shape
    k = w.shape[0]
    left, right = same_padding(k)
    emb = np.zeros((B, L + k - 1, table.shape[1]), dtype)
    emb[:, left:left + L] = table[tokens]
    conv = np.broadcast_to(b, (B, L, w.shape[2])).copy()
    for dk in range(k):
        if dtype is F64:
            conv += emb[:, dk:dk + L] @ w[dk]
        else:                                 # one term at a time, as a plain fp32 loop sums (BLAS blocks the sum and is closer)
            for e in range(w.shape[1]):
                conv += emb[:, dk:dk + L, e:e + 1] * w[dk, e]
    return emb, conv


def conv_pool_fwd(tokens, table, w, b, pool, dtype=F64):
    """-> (pooled [B, L // pool, F], arg-max index in the window [B, T', F] (lowest among ties), conv pre-activation)."""
    _, conv = conv_same(tokens, table, w, b, dtype)
    B, L, F = conv.shape
    T = L // pool
    y = np.maximum(conv[:, :T * pool], dtype(0.0)).reshape(B, T, pool, F)
    return y.max(axis=2), y.argmax(axis=2), conv


def conv_pool_bwd(tokens, table, w, b, pool, g, dtype=F64):
    """d pooled [B, T', F] -> (d table, d w, d b)."""
    tokens = np.asarray(tokens)
    emb, conv = conv_same(tokens, table, w, b, dtype)
    w = np.asarray(w, dtype)
    B, L, F = conv.shape
    k = w.shape[0]
    T = L // pool
    y = np.maximum(conv[:, :T * pool], dtype(0.0)).reshape(B, T, pool, F)
    arg = y.argmax(axis=2)
    dy = np.zeros((B, T, pool, F), dtype)
    bi, ti, fi = np.meshgrid(np.arange(B), np.arange(T), np.arange(F), indexing="ij")
    dy[bi, ti, arg, fi] = np.asarray(g, dtype)
    dconv = np.zeros((B, L, F), dtype)
    dconv[:, :T * pool] = dy.reshape(B, T * pool, F) * (conv[:, :T * pool] > 0)
    db = dconv.sum(axis=(0, 1))
    dw = np.stack([np.einsum("ble,blf->ef", emb[:, dk:dk + L], dconv) for dk in range(k)])
    demb = np.zeros_like(emb)
    for dk in range(k):
        demb[:, dk:dk + L] += dconv @ w[dk].T
    left, _ = same_padding(k)
    dtable = np.zeros(np.asarray(table).shape, dtype)
    np.add.at(dtable, tokens.reshape(-1), demb[:, left:left + L].reshape(B * L, -1))
    return dtable, dw, db


def conv_pool_loop(tokens, table, w, b, pool):
    """Literal loop transcription of the same layers (one output at a time), for small cases."""
    tokens = np.asarray(tokens)
    table, w, b = np.asarray(table, F64), np.asarray(w, F64), np.asarray(b, F64)
    B, L = tokens.shape
    k, E, F = w.shape
    left = (k - 1) // 2
    T = L // pool
    out = np.zeros((B, T, F), F64)
    for bb in range(B):
        for t in range(T):
            for f in range(F):
                best = None
                for j in range(pool):
                    c = t * pool + j
                    s = b[f]
                    for dk in range(k):
                        l = c + dk - left
                        if 0 <= l < L:
                            for e in range(E):
                                s += table[tokens[bb, l], e] * w[dk, e, f]
                    v = max(s, 0.0)
                    if best is None or v > best:
                        best = v
                out[bb, t, f] = best
    return out


# ---- LSTM(go_backwards=True) -----------------------------------------------------------------------------------------------
def lstm_fwd(x, wx, wh, b, act="hard_sigmoid", dtype=F64):
    """x [B, T, D] -> (h after input step 0 [B, H], cache for lstm_bwd)."""
    x, wx, wh, b = (np.asarray(t, dtype) for t in (x, wx, wh, b))
    B, T, _ = x.shape
    H = wh.shape[0]
    ra, _ = _rec(act, dtype)
    h, c = np.zeros((B, H), dtype), np.zeros((B, H), dtype)
    zs, cs, hs = [None] * T, [None] * T, [None] * T
    for t in reversed(range(T)):
        z = x[:, t] @ wx + h @ wh + b
        i, f, g, o = ra(z[:, :H]), ra(z[:, H:2 * H]), np.tanh(z[:, 2 * H:3 * H]), ra(z[:, 3 * H:])
        c = f * c + i * g
        h = o * np.tanh(c)
        zs[t], cs[t], hs[t] = z, c, h
    return h, (x, wx, wh, b, act, zs, cs, hs)


def lstm_bwd(cache, dh):
    """d h_final -> (dx [B, T, D], d wx, d wh, d b), in the dtype of the cache."""
    x, wx, wh, b, act, zs, cs, hs = cache
    B, T, D = x.shape
    H = wh.shape[0]
    dtype = x.dtype.type
    ra, rg = _rec(act, dtype)
    dh = np.asarray(dh, dtype).copy()
    dc = np.zeros((B, H), dtype)
    dx = np.zeros_like(x)
    dwx, dwh, db = np.zeros_like(wx), np.zeros_like(wh), np.zeros_like(b)
    for t in range(T):                       # reverse of the processing order
        z, c = zs[t], cs[t]
        cp = cs[t + 1] if t + 1 < T else np.zeros_like(c)
        hp = hs[t + 1] if t + 1 < T else np.zeros_like(c)
        zi, zf, zg, zo = z[:, :H], z[:, H:2 * H], z[:, 2 * H:3 * H], z[:, 3 * H:]
        i, f, g, o = ra(zi), ra(zf), np.tanh(zg), ra(zo)
        tc = np.tanh(c)
        dc = dc + dh * o * (1 - tc * tc)
        dz = np.concatenate([dc * g * rg(zi, i), dc * cp * rg(zf, f), dc * i * (1 - g * g), dh * tc * rg(zo, o)], axis=1)
        dx[:, t] = dz @ wx.T
        dwx += x[:, t].T @ dz
        dwh += hp.T @ dz
        db += dz.sum(axis=0)
        dh = dz @ wh.T
        dc = dc * f
    return dx, dwx, dwh, db


def lstm_loop(x, wx, wh, b, act="hard_sigmoid"):
    """Literal per-sequence, per-unit transcription of the Keras v1 cell with go_backwards (small cases)."""
    x, wx, wh, b = (np.asarray(t, F64) for t in (x, wx, wh, b))
    B, T, D = x.shape
    H = wh.shape[0]
    ra, _ = _rec(act)
    out = np.zeros((B, H), F64)
    for bb in range(B):
        h, c = [0.0] * H, [0.0] * H
        for t in range(T - 1, -1, -1):
            z = [b[n] + sum(x[bb, t, k] * wx[k, n] for k in range(D)) + sum(h[j] * wh[j, n] for j in range(H)) for n in range(4 * H)]
            nh, nc = [0.0] * H, [0.0] * H
            for u in range(H):
                i, f = float(ra(z[u])), float(ra(z[H + u]))
                g, o = np.tanh(z[2 * H + u]), float(ra(z[3 * H + u]))
                nc[u] = f * c[u] + i * g
                nh[u] = o * np.tanh(nc[u])
            h, c = nh, nc
        out[bb] = h
    return out


# ---- the whole model -----------------------------------------------------------------------------------------------------
PARAM_NAMES = ("conv_w", "conv_b", "dense_w", "dense_b", "embeddings", "conv_kernel", "conv_bias", "kernel", "recurrent_kernel",
               "bias", "hidden_w", "hidden_b", "out_w", "out_b")


def model_fwd(p, features, adjs, tokens, labels, mask, act="hard_sigmoid", pool=4):
    """p: dict of PARAM_NAMES (conv_w / conv_b: lists over adjacency channels).  -> (logits, cost_opt, cost_sum, cache)."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import kgcn_oracle as K
    x = np.asarray(features, F64)
    conv = K.graphconv_fwd(x, adjs, p["conv_w"], p["conv_b"])
    s1 = sigmoid(conv)
    s2 = sigmoid(s1 @ np.asarray(p["dense_w"], F64) + np.asarray(p["dense_b"], F64))
    graph = s2.sum(axis=1)
    pooled = conv_pool_fwd(tokens, p["embeddings"], p["conv_kernel"], p["conv_bias"], pool)[0]
    seq, lcache = lstm_fwd(pooled, p["kernel"], p["recurrent_kernel"], p["bias"], act)
    cat = np.concatenate([seq, graph], axis=1)
    pre = cat @ np.asarray(p["hidden_w"], F64) + np.asarray(p["hidden_b"], F64)
    hid = np.maximum(pre, 0.0)
    logits = hid @ np.asarray(p["out_w"], F64) + np.asarray(p["out_b"], F64)
    lab, m = np.asarray(labels, F64), np.asarray(mask, F64).reshape(-1)
    zmax = logits.max(axis=1, keepdims=True)
    lse = zmax[:, 0] + np.log(np.exp(logits - zmax).sum(axis=1))
    cost = m * (lse * lab.sum(axis=1) - (lab * logits).sum(axis=1))
    cache = (x, adjs, conv, s1, s2, cat, pre, hid, logits, lab, m, lcache, tokens, pool, K)
    return logits, cost.mean(), cost.sum(), cache


def model_bwd(p, cache):
    """Gradients of cost_opt with respect to every parameter: dict of PARAM_NAMES."""
    x, adjs, conv, s1, s2, cat, pre, hid, logits, lab, m, lcache, tokens, pool, K = cache
    B = logits.shape[0]
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    sm = e / e.sum(axis=1, keepdims=True)
    dlog = (m / B)[:, None] * (sm * lab.sum(axis=1, keepdims=True) - lab)
    g = {"out_w": hid.T @ dlog, "out_b": dlog.sum(axis=0)}
    dpre = (dlog @ np.asarray(p["out_w"], F64).T) * (pre > 0)
    g["hidden_w"], g["hidden_b"] = cat.T @ dpre, dpre.sum(axis=0)
    dcat = dpre @ np.asarray(p["hidden_w"], F64).T
    H = lcache[2].shape[0]
    dseq, dgraph = dcat[:, :H], dcat[:, H:]
    dx, g["kernel"], g["recurrent_kernel"], g["bias"] = lstm_bwd(lcache, dseq)
    g["embeddings"], g["conv_kernel"], g["conv_bias"] = conv_pool_bwd(tokens, p["embeddings"], p["conv_kernel"], p["conv_bias"], pool, dx)
    ds2 = np.broadcast_to(dgraph[:, None, :], s2.shape) * s2 * (1 - s2)
    g["dense_w"] = np.einsum("bnd,bne->de", s1, ds2)
    g["dense_b"] = ds2.sum(axis=(0, 1))
    dconv = (ds2 @ np.asarray(p["dense_w"], F64).T) * s1 * (1 - s1)
    _, dw, dbias = K.graphconv_bwd(x, adjs, p["conv_w"], p["conv_b"], dconv)
    g["conv_w"], g["conv_b"] = [np.asarray(t) for t in dw], [np.asarray(t).reshape(-1) for t in dbias]
    return g
