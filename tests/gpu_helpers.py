"""What several GPU test files need in the same form, in one copy: host <-> device conversions, the activations in fp64 by name,
the model of tests/golden/g7_sample_multimodal.npz with its oracle inputs (test_gpu_multimodal_ig.py, test_gpu_smooth_ig.py)
and the loaders of a Dense+BN layer's parameters (test_gpu_vecmodal.py, test_gpu_vecmodal_ig.py).  torch is imported by the
functions that need it, so that the module imports without one."""
import os

import numpy as np

import multimodal_ig_oracle as IG

G7_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g7_sample_multimodal.npz")


# ---- conversions ----------------------------------------------------------------------------------------------------------------------
def to_device(a, dtype=np.float32):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype), device="cuda")


def to_f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


# ---- activations in fp64, by name (None or anything else: the identity) ------------------------------------------------------------
def act64(v, act):
    if act == "sigmoid":
        return 1.0 / (1.0 + np.exp(-v))
    if act == "relu":
        return np.maximum(v, 0)
    if act == "tanh":
        return np.tanh(v)
    return v


def dact64(a, act):
    """The derivative formed from the activation's OUTPUT a, as the backward kernels form it."""
    if act == "sigmoid":
        return a * (1 - a)
    if act == "relu":
        return (a > 0).astype(np.float64)
    if act == "tanh":
        return 1 - a * a
    return np.ones_like(a)


# ---- the g7 multimodal model and its oracle inputs -----------------------------------------------------------------------------------
def conv_case(rng, C, L, E, k, p, S=7, F=50):
    import torch
    tok = rng.integers(0, S, size=(C, L)).astype(np.int32)
    table = rng.uniform(-1, 1, (S, E)).astype(np.float32)
    w = (rng.standard_normal((k, E, F)) / np.sqrt(k * E)).astype(np.float32)
    b = (rng.standard_normal(F) * 0.3).astype(np.float32)
    return torch.as_tensor(tok, device="cuda"), table, w, b, tok


def g7_case(E=4, seed=0):
    import torch
    from kgcn_amd import data_util as D, models
    g = np.load(G7_GOLDEN)
    channels, _ = D.build_adjs({"dense_adj": g["dense_adj"], "max_node_num": int(g["max_node_num"])})
    tokens, S = D.sequence_table({"sequence": g["sequence"], "sequence_symbol_num": g["sequence_symbol_num"]}, "cuda")
    dataset = D.DeviceGraphDataset(channels, g["feature"], device="cuda")
    torch.manual_seed(seed)
    model = models.MultimodalGCN(S, embedding_dim=E, adj_channel_num=len(channels), label_dim=2).cuda()
    with torch.no_grad():                              # larger embeddings than Keras' U(-0.05, 0.05): visible attributions
        model.sequence.embeddings.uniform_(-1.0, 1.0)
    adj, x = dataset.batch(np.arange(dataset.num_graphs))
    model(x, adj, sequences=tokens)
    return g, channels, dataset, tokens, model


def multimodal_params(model):
    _np = to_f64
    return {"conv_w": [_np(w) for w in model.conv.w], "conv_b": [_np(b).reshape(-1) for b in model.conv.bias],
            "dense_w": _np(model.dense.kernel), "dense_b": _np(model.dense.bias), "conv_kernel": _np(model.sequence.conv_kernel),
            "conv_bias": _np(model.sequence.conv_bias), "kernel": _np(model.sequence.kernel),
            "recurrent_kernel": _np(model.sequence.recurrent_kernel), "bias": _np(model.sequence.bias),
            "hidden_w": _np(model.hidden.kernel), "hidden_b": _np(model.hidden.bias), "out_w": _np(model.out.kernel),
            "out_b": _np(model.out.bias)}


def oracle_inputs(channels, features, tokens, table, b, N):
    adjs = [[]]
    for c in channels:
        sel = c.graph == b
        adjs[0].append((np.stack([c.row[sel], c.col[sel]], 1), c.val[sel].astype(np.float64), [N, N]))
    A, Sm = IG.dense_adjs(adjs, N)
    return np.asarray(features[b], np.float64), A[0], Sm[0], table[tokens[b]]


# ---- parameters of a Dense+BN layer from an oracle's dictionary ----------------------------------------------------------------------
def set_param(param, value):
    import torch
    with torch.no_grad():
        param.copy_(torch.as_tensor(np.asarray(value, np.float32), device=param.device).reshape(param.shape))


def load_dense_bn(layer, p):
    set_param(layer.kernel, p["w"])
    set_param(layer.bias, p["b"])
    if "gamma" in p:
        set_param(layer.gamma, p["gamma"]); set_param(layer.beta, p["beta"])
        set_param(layer.moving_mean, p["mean"]); set_param(layer.moving_variance, p["var"])
