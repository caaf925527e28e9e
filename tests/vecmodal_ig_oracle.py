"""numpy fp64 statement of visualization.vecmodal_integrated_gradients, built on tests/vecmodal_oracle.py.

  * the input gradients (d node features, d dense adjacency, d vector) of the score of models.MultimodalVecGCN (softmax
    probability of the target class) and models.MultimodalRegressionGCN (the prediction column), one compound at a time;
    tests/test_vecmodal_ig_oracle.py checks them against central differences
  * literal(): the loop of kgcn/visualization.py:187-260 as written there -- one forward + backward per step, IG += grad * data / D
    -- for 'ig', 'grad_prod', 'grad', and for 'smooth_grad' / 'smooth_ig' with the N(0, 1) noise passed in
  * closed_form(): the same attribution with the vector branch's first layer taken from P = v W (expand) and its gradient summed
    over the copies before ONE product with W^T (reduce) -- what csrc/vecig.hip computes
  * expand() / reduce(): the two sweeps themselves, for the kernels' own tests

Adjacency is dense [N, N]; the gradient with respect to it is reported on the stored (non-zero) entries only, as the device path
differentiates the stored values of channel 0.  BatchNormalization runs in learning phase 0."""
import numpy as np

import smooth_ig_oracle as SO
import vecmodal_oracle as O

F64 = np.float64
STREAM_VECTOR = 0x200
CLEAN = ("ig", "grad_prod", "grad")
SMOOTH = ("smooth_grad", "smooth_ig")


def modal_targets(kind, modal, vector_name=None):
    name = vector_name or ("dragon" if kind == "regression" else "profeat")
    modals = ("features", name) if kind == "regression" else ("features", "adjs", name)
    if modal == "all":
        return modals, name
    if modal not in modals:
        raise ValueError(modal)
    return (modal,), name


# ---- the two sweeps ---------------------------------------------------------------------------------------------------------------
def bn_constants(p, eps=1e-3):
    """-> (scale, shift) of a dense_bn parameter dict: bn(x) = scale x + shift (ones and zeros without normalisation)."""
    n = np.asarray(p["w"]).shape[1]
    if "gamma" not in p:
        return np.ones(n), np.zeros(n)
    scale = np.asarray(p["gamma"], F64) / np.sqrt(np.asarray(p["var"], F64) + eps)
    return scale, np.asarray(p["beta"], F64) - scale * np.asarray(p["mean"], F64)


def expand(Pm, alpha, bias, scale, shift, act):
    """Y[c K + k] = act(scale (alpha[k] P[c] + bias) + shift): P [C, H] -> [C K, H]"""
    Pm, alpha = np.asarray(Pm, F64), np.asarray(alpha, F64)
    pre = alpha[None, :, None] * Pm[:, None, :] + np.asarray(bias, F64)
    return O.act_fwd(np.asarray(scale, F64) * pre + np.asarray(shift, F64), act).reshape(-1, Pm.shape[1])


def reduce(dY, Y, w, scale, act):
    """S[c] = scale sum_k w[k] dY[c K + k] act'(Y[c K + k]); a copy of weight 0 is left out whatever its dY holds"""
    w = np.asarray(w, F64)
    K = w.shape[0]
    dY, Y = np.asarray(dY, F64).reshape(-1, K, np.shape(Y)[1]), np.asarray(Y, F64).reshape(-1, K, np.shape(Y)[1])
    S = np.zeros((Y.shape[0], Y.shape[2]))
    for k in range(K):
        if w[k] != 0:
            S += w[k] * dY[:, k] * O.act_grad(Y[:, k], act)
    return S * np.asarray(scale, F64)


# ---- score and input gradients, one compound ------------------------------------------------------------------------------------------
def _first_layer(kind, P):
    return P["vec"] if kind == "regression" else P["tower"][0]


def score_grads(kind, P, x, A, v, mask, size=None, first=None, pres=None):
    """-> (score, {"features": d x [N, F], "adjs": d A [N, N] on the stored entries, "vector": d v [Dv], "first": d score / d
    first-layer output [H]}).  mask [K] selects the class(es) / prediction column(s).  first [H]: the output of the vector
    branch's first layer in place of v (then "vector" is None).  pres: a list that receives (layer name, relu pre-activation)."""
    x, A, mask = np.asarray(x, F64)[None], np.asarray(A, F64), np.asarray(mask, F64)
    fl = _first_layer(kind, P)
    if first is None:
        v = np.asarray(v, F64)[None]
        y1 = O.dense_bn_fwd(v, fl, "relu")
    else:
        y1 = np.asarray(first, F64)[None]

    def note(name, xin, p):
        if pres is not None:
            pres.append((name, O.dense_bn_fwd(xin, p, None)))

    if first is None:
        note("first", v, fl)
    if kind == "vec":
        xw = x[0] @ np.asarray(P["conv"]["w"], F64) + np.asarray(P["conv"]["b"], F64)
        h1 = O.act_fwd(A @ xw, "sigmoid")
        wd = np.asarray(P["dense"]["w"], F64)
        h2 = O.act_fwd(h1 @ wd + np.asarray(P["dense"]["b"], F64), "sigmoid")
        graph = h2.sum(axis=0)[None]
        t = [y1]
        for i, p in enumerate(P["tower"][1:]):
            note("tower%d" % (i + 1), t[-1], p)
            t.append(O.dense_bn_fwd(t[-1], p, "relu"))
        joined = np.concatenate([t[-1], graph], axis=1)
        note("hidden", joined, P["hidden"])
        hid = O.dense_bn_fwd(joined, P["hidden"], "relu")
        logits = O.dense_bn_fwd(hid, P["out"], None)
        e = np.exp(logits - logits.max())
        prob = e / e.sum()
        score = float((prob * mask).sum())
        dlog = prob * (mask - score)
        g = O.dense_bn_bwd(hid, P["out"], dlog, None)["x"]
        g = O.dense_bn_bwd(joined, P["hidden"], g, "relu")["x"]
        vw = t[-1].shape[1]
        dvec, dgraph = g[:, :vw], g[:, vw:]
        for i in (2, 1):
            dvec = O.dense_bn_bwd(t[i - 1], P["tower"][i], dvec, "relu")["x"]
        dz2 = np.broadcast_to(dgraph, h2.shape) * O.act_grad(h2, "sigmoid")
        dz1 = (dz2 @ wd.T) * O.act_grad(h1, "sigmoid")
        dx = (A.T @ dz1) @ np.asarray(P["conv"]["w"], F64).T
        dA = np.where(A != 0, dz1 @ xw.T, 0.0)
    else:
        N = x.shape[1]
        sizes = np.array([N if size is None else int(size)])
        acts = ("relu", "relu", None)
        ins, pre_l = [x], []
        for i in range(3):
            pre = ins[-1] @ np.asarray(P["gd"][i]["w"], F64) + np.asarray(P["gd"][i]["b"], F64)
            pre_l.append(pre)
            y, valid = O._graph_bn(pre, P["bn"][i], sizes, acts[i])
            if pres is not None and acts[i] == "relu":
                pres.append(("graph%d" % i, O._graph_bn(pre, P["bn"][i], sizes, None)[0][valid[..., 0]]))
            ins.append(y)
        graph = np.tanh(ins[-1].sum(axis=1))
        joined = np.concatenate([y1, graph], axis=1)
        pred = O.dense_bn_fwd(joined, P["out"], None)
        score = float((pred * mask).sum())
        g = O.dense_bn_bwd(joined, P["out"], mask[None], None)["x"]
        vw = y1.shape[1]
        dvec = g[:, :vw]
        d = np.broadcast_to((g[:, vw:] * (1.0 - graph * graph))[:, None, :], ins[-1].shape)
        for i in reversed(range(3)):
            dpre, _ = O._graph_bn_bwd(pre_l[i], P["bn"][i], sizes, acts[i], d)
            d = dpre @ np.asarray(P["gd"][i]["w"], F64).T
        dx, dA = d[0], np.zeros_like(A)
    dv = None if first is not None else O.dense_bn_bwd(v, fl, dvec, "relu")["x"][0]
    return score, {"features": dx, "adjs": dA, "vector": dv, "first": dvec[0]}


def host_noise(seed, g, D, x_shape, A, Dv):
    """The N(0, 1) values the device draws for compound g, samples 0 .. D - 1 (include/kgcn_hip.h, restated by
    smooth_ig_oracle.noise): the features [N, F], the stored entries of adjacency channel 0 in CSR order, the vector as [1, Dv]."""
    idx = np.argwhere(np.asarray(A) != 0)
    out = {"features": np.zeros((D,) + tuple(x_shape)), "adjs": np.zeros((D,) + np.shape(A)), "vector": np.zeros((D, Dv))}
    for k in range(D):
        out["features"][k] = SO.noise(seed, SO.STREAM_FEATURES, g, k, *x_shape)
        out["adjs"][k][idx[:, 0], idx[:, 1]] = SO.noise(seed, SO.STREAM_ADJACENCY, g, k, 1, len(idx))[0]
        out["vector"][k] = SO.noise(seed, STREAM_VECTOR, g, k, 1, Dv)[0]
    return out


def scales_weights(method, D):
    """The copies of one compound -> (scales, weights, noisy, start_row, end_row): ig_scales / smooth_rows of the implementation."""
    D = int(D)
    if method == "ig":
        return [k / D for k in range(D + 1)], [0.0] + [1.0 / D] * D, False, 0, D
    if method in ("grad_prod", "grad"):
        return [0.0, 1.0], [0.0, 1.0], False, 0, 1
    if method in SMOOTH:
        return [0.0, 1.0] + [1.0 if method == "smooth_grad" else (k + 1) / D for k in range(D)], [0.0, 0.0] + [1.0 / D] * D, True, 0, 1
    raise ValueError(method)


def _record(targets, name, data, ig, start, end):
    rec = {"start": start, "end": end}
    for m in targets:
        key = "vector" if m == name else m
        rec[m + "_IG"] = ig[key][None] if m == name else ig[key]
        rec[m] = data[key]
    rec["sum_of_IG"] = float(sum(rec[m + "_IG"].sum() for m in targets))
    return rec


def literal(kind, P, x, A, v, mask, modal, method, D, size=None, noise=None, noise_scale=0.1, vector_name=None, pres=None):
    """kgcn/visualization.py:187-260 for one compound.  The inputs named by `modal` are scaled by k / D for k = 1 .. D and the
    gradient of the score with respect to them is taken at every step: IG[m] += grad * data / D ('ig'); 'grad_prod' / 'grad': one
    step at scale 1, grad * data / grad.  'smooth_grad' / 'smooth_ig' (:235-259): step k feeds data * s_k + noise_scale * z_k with
    s_k = 1 (smooth_grad) or (k + 1) / D (smooth_ig) and noise = {"features": z [D, N, F], "adjs": z [D, N, N] (zero off the stored entries), "vector":
    z [D, Dv]}: IG[m] += grad / D (* data for smooth_ig).  start / end: the score of the clean inputs at scale 0 and 1."""
    targets, name = modal_targets(kind, modal, vector_name)
    data = {"features": np.asarray(x, F64), "adjs": np.asarray(A, F64), "vector": np.asarray(v, F64)}
    keys = ["vector" if m == name else m for m in targets]

    def fed(scale, k=None):
        f = dict(data)
        for m in keys:
            f[m] = data[m] * scale
            if k is not None:
                f[m] = f[m] + noise_scale * np.asarray(noise[m][k], F64)
        return f

    def run(f, note=None):
        return score_grads(kind, P, f["features"], f["adjs"], f["vector"], mask, size, pres=note)

    ig = {m: np.zeros_like(data[m]) for m in keys}
    D = int(D)
    if method == "ig":
        for k in range(D):
            _, g = run(fed((k + 1) / D), pres)
            for m in keys:
                ig[m] += g[m] * data[m] / D
    elif method in ("grad_prod", "grad"):
        _, g = run(fed(1.0), pres)
        for m in keys:
            ig[m] += g[m] * data[m] if method == "grad_prod" else g[m]
    elif method in SMOOTH:
        for k in range(D):
            _, g = run(fed(1.0 if method == "smooth_grad" else (k + 1) / D, k), pres)
            for m in keys:
                ig[m] += g[m] * data[m] / D if method == "smooth_ig" else g[m] / D
    else:
        raise ValueError(method)
    start, end = run(fed(0.0))[0], run(fed(1.0))[0]
    return _record(targets, name, data, ig, start, end)


def closed_form(kind, P, x, A, v, mask, modal, method, D, size=None, noise=None, noise_scale=0.1, vector_name=None):
    """The same attribution the way the fused route forms it: the first layer of every clean copy from P = v W by expand(), the
    first layer of a noisy copy from the layer itself; the gradient at the first layer's output of every copy, reduce() over the
    copies, ONE product with W^T, times v.  The graph branch is the literal loop's."""
    targets, name = modal_targets(kind, modal, vector_name)
    data = {"features": np.asarray(x, F64), "adjs": np.asarray(A, F64), "vector": np.asarray(v, F64)}
    keys = ["vector" if m == name else m for m in targets]
    scales, weights, noisy, start_row, end_row = scales_weights(method, D)
    fl = _first_layer(kind, P)
    W = np.asarray(fl["w"], F64)
    scale, shift = bn_constants(fl)
    K = len(scales)
    if "vector" not in keys:
        Y = np.repeat(O.dense_bn_fwd(data["vector"][None], fl, "relu"), K, axis=0)
    elif not noisy:
        Y = expand((data["vector"] @ W)[None], scales, fl["b"], scale, shift, "relu")
    else:
        rows = [data["vector"] * s + (noise_scale * np.asarray(noise["vector"][k - 2], F64) if k >= 2 else 0.0) for k, s in enumerate(scales)]
        Y = O.dense_bn_fwd(np.stack(rows), fl, "relu")
    ig = {m: np.zeros_like(data[m]) for m in keys}
    dY = np.full_like(Y, np.nan)                                    # the rows of weight-0 copies are never filled in
    score = np.zeros(K)
    for k, (s, w) in enumerate(zip(scales, weights)):
        f = dict(data)
        for m in keys:
            if m != "vector":
                f[m] = data[m] * s + (noise_scale * np.asarray(noise[m][k - 2], F64) if noisy and k >= 2 else 0.0)
        score[k], g = score_grads(kind, P, f["features"], f["adjs"], None, mask, size, first=Y[k])
        if w != 0:
            dY[k] = g["first"]
            for m in keys:
                if m != "vector":
                    ig[m] += w * g[m]
    if "vector" in keys:
        ig["vector"] = reduce(dY, Y, weights, scale, "relu")[0] @ W.T
    if method not in ("grad", "smooth_grad"):
        for m in keys:
            ig[m] = ig[m] * data[m]
    return _record(targets, name, data, ig, float(score[start_row]), float(score[end_row]))


def relu_margins(kind, P, x, A, v, mask, modal, method, D, size=None, noise=None, noise_scale=0.1):
    """-> {layer: (min |pre| over the relu units of the copies with non-zero weight, max |pre|)} of the literal loop"""
    pres = []
    literal(kind, P, x, A, v, mask, modal, method, D, size, noise, noise_scale, pres=pres)
    out = {}
    for name, pre in pres:
        a = np.abs(pre)
        lo, hi = out.get(name, (np.inf, 0.0))
        out[name] = (min(lo, float(a.min())), max(hi, float(a.max())))
    return out


# ---- the cases the tests share ----------------------------------------------------------------------------------------------------------
# Parameter seeds whose relu units all keep |pre| >= 1e-5 of their layer's largest |pre| on every copy of non-zero weight, for every
# modal and method at D = 8 on the first five compounds of g12_vecmodal.npz (tests/test_vecmodal_ig_oracle.py asserts it): a unit
# closer to zero may switch its derivative between fp32 and fp64.
PARAM_SEEDS = {"vec": 7, "regression": 8}
DIVIDE, NOISE_SEED, NOISE_SCALE, COMPOUNDS = 8, 1234, 0.1, (0, 1, 2, 3, 4)
METHODS = CLEAN + SMOOTH


def case(kind, Z):
    """-> (parameters, features [G, N, F], dense adjacency [G, N, N], vectors [G, Dv], sizes [G] or None) of the fixture Z"""
    rng = np.random.default_rng(PARAM_SEEDS[kind])
    F = Z["ds_feature"].shape[2]
    if kind == "vec":
        return O.draw_vec_model(rng, F, Z["ds_profeat"].shape[1]), Z["ds_feature"], Z["ds_dense_adj"].astype(F64), Z["ds_profeat"], None
    return (O.draw_regression_model(rng, F, Z["ds_dragon"].shape[1]), Z["ds_feature"], Z["ds_dense_adj"].astype(F64), Z["ds_dragon"],
            Z["ds_sizes"])
