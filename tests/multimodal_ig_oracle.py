"""fp64 restatement of integrated gradients for the multimodal model (kgcn/visualization.py:187-285, CompoundVisualizer on
example_model/model_multimodal.py built with feed_embedded_layer=True, gcn.py:637-656).  Builds on tests/multimodal_oracle.py
(imported, not edited) and extends its backward to the three inputs the reference integrates over: the node features, the values
of adjacency channel 0 and the embedded protein sequence (the `embedded_layer` placeholder, fed in place of the Embedding).

  inputs      x [B, N, F], A [B, C, N, N] dense adjacency (the stored entries), emb [B, L, E] the embedded sequence
  prediction  softmax(logits) (model_multimodal.py:106); the score is sum_k mask[k] prediction[k] (one class, or all of them)
  IG          kgcn/feed.py:116-121, 126-131, 219-232: every input named in the modal set is scaled by s (the values of every
              adjacency channel); the gradient is taken with respect to the scaled placeholder (channel-0 values for adjs)

Every function computes in float64 (the two conv-pool functions in fp32 when given dtype=np.float32, as in multimodal_oracle)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multimodal_oracle as M  # noqa: E402

F64 = np.float64
MODALS = ("features", "adjs", "embedded_layer")


def dense_adjs(adjs, N):
    """adjs[b][c] = (idx [nnz, 2], values, shape) -> (A [B, C, N, N], stored-entry mask [B, C, N, N])."""
    B, C = len(adjs), len(adjs[0])
    A, S = np.zeros((B, C, N, N), F64), np.zeros((B, C, N, N), bool)
    for b in range(B):
        for c in range(C):
            idx, val = np.asarray(adjs[b][c][0]).reshape(-1, 2), np.asarray(adjs[b][c][1], F64)
            np.add.at(A[b, c], (idx[:, 0], idx[:, 1]), val)
            S[b, c, idx[:, 0], idx[:, 1]] = True
    return A, S


def conv_pool_fwd_emb(emb, w, b, pool, dtype=F64):
    """Conv1D(same, relu) + MaxPooling1D on the embedded input [B, L, E] -> (pooled, arg-max (lowest on ties), conv)."""
    emb, w, b = np.asarray(emb, dtype), np.asarray(w, dtype), np.asarray(b, dtype)
    B, L, E = emb.shape
    k = w.shape[0]
    left, _ = M.same_padding(k)
    pad = np.zeros((B, L + k - 1, E), dtype)
    pad[:, left:left + L] = emb
    conv = np.broadcast_to(b, (B, L, w.shape[2])).copy()
    for dk in range(k):
        if dtype is F64:
            conv += pad[:, dk:dk + L] @ w[dk]
        else:                                 # one term at a time, as in multimodal_oracle.conv_same
            for e in range(E):
                conv += pad[:, dk:dk + L, e:e + 1] * w[dk, e]
    T = L // pool
    y = np.maximum(conv[:, :T * pool], dtype(0.0)).reshape(B, T, pool, -1)
    return y.max(axis=2), y.argmax(axis=2), conv


def conv_pool_input_grad(conv, arg, w, pool, g, dtype=F64):
    """d pooled [B, T, F] -> d emb [B, L, E]: routed to the arg-max position (nothing where the maximum is not > 0), then
    demb[m, e] = sum_j sum_f dconv[m + padL - j, f] w[j, e, f]."""
    w = np.asarray(w, dtype)
    B, L, F = conv.shape
    k = w.shape[0]
    T = np.asarray(g).shape[1]
    dy = np.zeros((B, T, pool, F), dtype)
    bi, ti, fi = np.meshgrid(np.arange(B), np.arange(T), np.arange(F), indexing="ij")
    dy[bi, ti, arg, fi] = np.asarray(g, dtype)
    dconv = np.zeros((B, L, F), dtype)
    dconv[:, :T * pool] = dy.reshape(B, T * pool, F) * (conv[:, :T * pool] > 0)
    left, _ = M.same_padding(k)
    dpad = np.zeros((B, L + k - 1, w.shape[1]), dtype)
    for dk in range(k):
        dpad[:, dk:dk + L] += dconv @ w[dk].T
    return dpad[:, left:left + L]


def forward(p, x, A, emb, act="hard_sigmoid", pool=4):
    """-> (prediction [B, K], cache)."""
    x, A = np.asarray(x, F64), np.asarray(A, F64)
    C = A.shape[1]
    fw = [x @ np.asarray(p["conv_w"][c], F64) + np.asarray(p["conv_b"][c], F64).reshape(-1) for c in range(C)]
    conv = sum(A[:, c] @ fw[c] for c in range(C))
    s1 = M.sigmoid(conv)
    s2 = M.sigmoid(s1 @ np.asarray(p["dense_w"], F64) + np.asarray(p["dense_b"], F64))
    graph = s2.sum(axis=1)
    pooled, arg, cconv = conv_pool_fwd_emb(emb, p["conv_kernel"], p["conv_bias"], pool)
    seq, lcache = M.lstm_fwd(pooled, p["kernel"], p["recurrent_kernel"], p["bias"], act)
    cat = np.concatenate([seq, graph], axis=1)
    pre = cat @ np.asarray(p["hidden_w"], F64) + np.asarray(p["hidden_b"], F64)
    hid = np.maximum(pre, 0.0)
    logits = hid @ np.asarray(p["out_w"], F64) + np.asarray(p["out_b"], F64)
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    prob = e / e.sum(axis=1, keepdims=True)
    return prob, (x, A, fw, s1, s2, pre, prob, lcache, arg, cconv, pool)


def backward(p, cache, dprob):
    """d prediction [B, K] -> (d x [B, N, F], d A [B, C, N, N], d emb [B, L, E])."""
    x, A, fw, s1, s2, pre, prob, lcache, arg, cconv, pool = cache
    dprob = np.asarray(dprob, F64)
    dlog = prob * (dprob - (dprob * prob).sum(axis=1, keepdims=True))
    dpre = (dlog @ np.asarray(p["out_w"], F64).T) * (pre > 0)
    dcat = dpre @ np.asarray(p["hidden_w"], F64).T
    H = lcache[2].shape[0]
    dseq, dgraph = dcat[:, :H], dcat[:, H:]
    dpooled = M.lstm_bwd(lcache, dseq)[0]
    demb = conv_pool_input_grad(cconv, arg, p["conv_kernel"], pool, dpooled)
    ds2 = np.broadcast_to(dgraph[:, None, :], s2.shape) * s2 * (1 - s2)
    dconv = (ds2 @ np.asarray(p["dense_w"], F64).T) * s1 * (1 - s1)
    C = A.shape[1]
    dA = np.stack([dconv @ fw[c].transpose(0, 2, 1) for c in range(C)], axis=1)
    dx = sum((A[:, c].transpose(0, 2, 1) @ dconv) @ np.asarray(p["conv_w"][c], F64).T for c in range(C))
    return dx, dA, demb


def scaled_inputs(x, A, emb, s, pert):
    return (x * s if "features" in pert else x, A * s if "adjs" in pert else A, emb * s if "embedded_layer" in pert else emb)


def input_grads(p, x, A, S, emb, mask, s, pert, act="hard_sigmoid", pool=4):
    """Score and gradients of one compound at scale s: {modal: gradient} (adjs: channel 0, at the stored entries)."""
    xs, As, es = scaled_inputs(x[None], A[None], emb[None], s, pert)
    prob, cache = forward(p, xs, As, es, act, pool)
    dx, dA, de = backward(p, cache, np.asarray(mask, F64)[None])
    return float((prob[0] * mask).sum()), {"features": dx[0], "adjs": dA[0, 0] * S[0], "embedded_layer": de[0]}


def integrated_gradients(p, x, A, S, emb, mask, divide_number=100, modal="all", method="ig", act="hard_sigmoid", pool=4):
    """The D + 1 scaled copies of one compound as the rows of ONE batch (what the GPU path does): x [N, F], A [C, N, N] with its
    stored-entry mask S, emb [L, E] -> {modal + '_IG': array, 'check_score', 'sum_of_IG', 'start_score', 'end_score'}."""
    pert = MODALS if modal == "all" else (modal,)
    D = int(divide_number)
    if method == "ig":
        scales, weights = np.arange(D + 1) / float(D), np.r_[0.0, np.full(D, 1.0 / D)]
    else:
        scales, weights = np.array([0.0, 1.0]), np.array([0.0, 1.0])
    R = len(scales)
    sx = scales.reshape(R, 1, 1)
    xs = x[None] * sx if "features" in pert else np.broadcast_to(x, (R,) + x.shape)
    As = A[None] * scales.reshape(R, 1, 1, 1) if "adjs" in pert else np.broadcast_to(A, (R,) + A.shape)
    es = emb[None] * sx if "embedded_layer" in pert else np.broadcast_to(emb, (R,) + emb.shape)
    prob, cache = forward(p, xs, As, es, act, pool)
    dx, dA, de = backward(p, cache, np.broadcast_to(np.asarray(mask, F64), prob.shape))
    g = {"features": np.tensordot(weights, dx, 1), "adjs": np.tensordot(weights, dA[:, 0], 1) * S[0],
         "embedded_layer": np.tensordot(weights, de, 1)}
    data = {"features": x, "adjs": A[0], "embedded_layer": emb}
    score = (prob * mask).sum(axis=1)
    out = {m + "_IG": (g[m] if method == "grad" else g[m] * data[m]) for m in pert}
    out["start_score"], out["end_score"] = float(score[0]), float(score[-1])
    out["check_score"] = out["end_score"] - out["start_score"]
    out["sum_of_IG"] = float(sum(out[m + "_IG"].sum() for m in pert))
    return out


def integrated_gradients_literal(p, x, A, S, emb, mask, divide_number=100, modal="all", method="ig", act="hard_sigmoid", pool=4):
    """Literal restatement of cal_integrated_gradients (:187-231) and check_IG (:277-285): one batch-1 pass per step."""
    pert = list(MODALS) if modal == "all" else [modal]
    data = {"features": x, "adjs": A[0], "embedded_layer": emb}
    IGs = {k: np.zeros(data[k].shape, F64) for k in pert}
    if method == "ig":
        for k in range(divide_number):
            scaling_coef = (k + 1) / float(divide_number)
            _, out_grads = input_grads(p, x, A, S, emb, mask, scaling_coef, pert, act, pool)
            for m in IGs:
                IGs[m] += out_grads[m] * data[m] / float(divide_number)
    elif method == "grad_prod":
        _, out_grads = input_grads(p, x, A, S, emb, mask, 1.0, pert, act, pool)
        for m in IGs:
            IGs[m] += out_grads[m] * data[m]
    elif method == "grad":
        _, out_grads = input_grads(p, x, A, S, emb, mask, 1.0, pert, act, pool)
        for m in IGs:
            IGs[m] += out_grads[m]
    else:
        raise ValueError(method)
    start = input_grads(p, x, A, S, emb, mask, 0.0, pert, act, pool)[0]
    end = input_grads(p, x, A, S, emb, mask, 1.0, pert, act, pool)[0]
    out = {m + "_IG": v for m, v in IGs.items()}
    out["start_score"], out["end_score"], out["check_score"] = start, end, end - start
    out["sum_of_IG"] = float(sum(v.sum() for v in IGs.values()))
    return out


def random_params(rng, S, E, F_in, C=1, K=2, H=32, scale=1.0):
    """Parameters of PARAM_NAMES at the model's widths (GraphConv 50, Dense 50, conv 50 x 4, LSTM 32, hidden 52)."""
    g = lambda *shape: rng.standard_normal(shape) * scale / np.sqrt(shape[-2] if len(shape) > 1 else 1.0)
    p = {"conv_w": [g(F_in, 50) for _ in range(C)], "conv_b": [rng.standard_normal(50) * 0.1 for _ in range(C)],
         "dense_w": g(50, 50), "dense_b": rng.standard_normal(50) * 0.1, "embeddings": rng.uniform(-1, 1, (S, E)),
         "conv_kernel": rng.standard_normal((4, E, 50)) / np.sqrt(4 * E), "conv_bias": rng.standard_normal(50) * 0.1,
         "kernel": g(50, 4 * H), "recurrent_kernel": g(H, 4 * H), "bias": np.r_[np.zeros(H), np.ones(H), np.zeros(2 * H)],
         "hidden_w": g(H + 50, 52), "hidden_b": rng.standard_normal(52) * 0.1, "out_w": g(52, K), "out_b": np.zeros(K)}
    return p
