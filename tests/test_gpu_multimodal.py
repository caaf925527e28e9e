"""The multimodal graph + sequence model on the GPU (csrc/seq.hip, ops.seq_conv_pool / ops.seq_lstm, models.MultimodalGCN) against
the fp64 oracle of tests/multimodal_oracle.py: the fused conv-pool and the go_backwards LSTM forward and backward over short,
odd and long sequences, the whole model on sample.jbl and at the compound-protein shape, reproducibility and the captured
training step.  Every comparison prints its error (max abs error / max abs reference value)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import multimodal_oracle as M  # noqa: E402
from family_bounds import rel_err  # noqa: E402
from gpu_helpers import to_device as _t, to_f64 as _np  # noqa: E402

pytestmark = pytest.mark.gpu

# max abs error / max abs fp64 value, for every T' here (up to 512): the largest errors measured on an MI355X were 4.3e-7 (pooled),
# 3.0e-7 (h), 3.6e-7 (dx), 4.3e-7 (d table), 3.5e-6 (d w, 717k routed positions), 1.1e-6 (d W_x), 7.1e-7 (d W_h), 8.9e-7 (LSTM
# bias); the long sequences need no wider bound
TOL = 1e-5
GOLDEN = os.path.join(ROOT, "tests", "golden", "g7_sample_multimodal.npz")


def _report(tag, errs, tol):
    print("%s: %s" % (tag, "  ".join("%s %.2e" % kv for kv in errs.items())))
    bad = {k: v for k, v in errs.items() if not v <= tol}
    assert not bad, (tag, bad, tol)


def _tokens(rng, B, L, S, kind):
    tok = rng.integers(0, S, size=(B, L)).astype(np.int32)
    if kind == "repeat":                    # runs of one token: identical conv outputs inside a pool window
        tok[:, :] = np.repeat(rng.integers(0, S, size=(B, (L + 7) // 8)), 8, axis=1)[:, :L]
    elif kind == "padding":                 # all padding (symbol 0)
        tok[:] = 0
    elif kind == "tail":                    # a short sequence padded with zeros
        tok[:, L // 3:] = 0
    return tok


def _encoder_params(rng, S, E, F=50, k=4, H=32):
    lim = np.sqrt(6.0 / (k * E + k * F))
    p = {"table": rng.uniform(-0.5, 0.5, (S, E)), "w": rng.uniform(-lim, lim, (k, E, F)), "b": rng.uniform(-0.1, 0.1, F),
         "wx": rng.uniform(-0.3, 0.3, (F, 4 * H)), "wh": np.linalg.qr(rng.standard_normal((4 * H, H)))[0].T,
         "bias": np.concatenate([np.zeros(H), np.ones(H), np.zeros(2 * H)]) + rng.uniform(-0.1, 0.1, 4 * H)}
    return {k_: v.astype(np.float32) for k_, v in p.items()}


CASES = [  # (B, L, E, kind, act)
    (1, 1, 4, "random", "hard_sigmoid"),          # L < k and T' = 0
    (17, 3, 25, "random", "sigmoid"),             # L < pool: T' = 0
    (1, 5, 4, "random", "hard_sigmoid"),          # L not a multiple of the pool
    (17, 5, 25, "padding", "sigmoid"),
    (17, 701, 25, "random", "hard_sigmoid"),
    (17, 701, 4, "repeat", "sigmoid"),
    (4097, 701, 25, "tail", "hard_sigmoid"),      # the compound-protein shape (+1 sequence)
    (17, 2048, 4, "random", "hard_sigmoid"),      # T' = 512
    (17, 2048, 25, "repeat", "sigmoid"),
]


@pytest.mark.parametrize("B,L,E,kind,act", CASES)
def test_encoder_forward_backward_against_oracle(B, L, E, kind, act):
    import torch
    from kgcn_amd import ops
    rng = np.random.default_rng(B * 7919 + L * 31 + E)
    S = 25
    p = _encoder_params(rng, S, E)
    tok = _tokens(rng, B, L, S, kind)
    T = L // 4
    # d pooled with a non-zero mean: zero-mean noise summed over B T' = 717k routed positions (d w, d b, d table) cancels to
    # ~1/800 of its absolute sum, and an fp32 sum of any order then misses a 1e-5 bound (measured 2.7e-4 .. 9.7e-4 at B = 4097)
    gp = (rng.standard_normal((B, T, 50)) + 1.0).astype(np.float32)
    gh = rng.standard_normal((B, 32)).astype(np.float32)
    tp = {k: _t(v).requires_grad_(True) for k, v in p.items()}
    ttok = torch.as_tensor(tok, device="cuda")
    pooled = ops.seq_conv_pool(ttok, tp["table"], tp["w"], tp["b"], 4)
    x = _t(_np(pooled)).requires_grad_(True)          # the LSTM gets its own leaf: both backward passes are checked separately
    h = ops.seq_lstm(x, tp["wx"], tp["wh"], tp["bias"], act)
    pooled.backward(_t(gp))
    h.backward(_t(gh))
    torch.cuda.synchronize()
    ref_pooled = M.conv_pool_fwd(tok, p["table"], p["w"], p["b"], 4)[0]
    dtab, dw, db = M.conv_pool_bwd(tok, p["table"], p["w"], p["b"], 4, gp)
    ref_h, cache = M.lstm_fwd(_np(pooled), p["wx"], p["wh"], p["bias"], act)
    dx, dwx, dwh, dbias = M.lstm_bwd(cache, gh)
    errs = {"pooled": rel_err(_np(pooled), ref_pooled) if T else 0.0, "h": rel_err(_np(h), ref_h)}
    if T:
        errs.update({"d_table": rel_err(_np(tp["table"].grad), dtab), "d_w": rel_err(_np(tp["w"].grad), dw), "d_b": rel_err(_np(tp["b"].grad), db),
                     "dx": rel_err(_np(x.grad), dx), "d_wx": rel_err(_np(tp["wx"].grad), dwx), "d_wh": rel_err(_np(tp["wh"].grad), dwh),
                     "d_bias": rel_err(_np(tp["bias"].grad), dbias)})
    else:
        assert tuple(pooled.shape) == (B, 0, 50)
        assert not np.any(_np(h)) and not np.any(_np(tp["table"].grad)) and not np.any(_np(tp["wx"].grad))
    _report("B=%d L=%d E=%d %s %s" % (B, L, E, kind, act), errs, TOL)


def test_no_grad_writes_only_the_final_h():
    import torch
    from kgcn_amd import ops
    rng = np.random.default_rng(3)
    p = _encoder_params(rng, 25, 4)
    tok = _tokens(rng, 9, 64, 25, "random")
    buf = torch.full((9, 40), 7.0, device="cuda")
    with torch.no_grad():
        pooled = ops.seq_conv_pool(torch.as_tensor(tok, device="cuda"), _t(p["table"]), _t(p["w"]), _t(p["b"]), 4)
        h = ops.seq_lstm(pooled, _t(p["wx"]), _t(p["wh"]), _t(p["bias"]), out=buf, out_col=5)
    ref = M.lstm_fwd(M.conv_pool_fwd(tok, p["table"], p["w"], p["b"], 4)[0], p["wx"], p["wh"], p["bias"])[0]
    assert h.data_ptr() == buf.data_ptr() + 20
    b = _np(buf)
    assert np.all(b[:, :5] == 7.0) and np.all(b[:, 37:] == 7.0)
    _report("no_grad h into columns 5..36", {"h": rel_err(b[:, 5:37], ref)}, TOL)


def test_sigmoid_lstm_matches_torch_nn_lstm():
    """nn.LSTM gate order i, f, g, o = Keras' i, f, c, o; weight_ih = kernel^T, weight_hh = recurrent_kernel^T, b_hh = 0;
    go_backwards = the time-reversed sequence."""
    import torch
    from kgcn_amd import ops
    rng = np.random.default_rng(5)
    B, T, D, H = 33, 150, 50, 32
    x = rng.standard_normal((B, T, D)).astype(np.float32)
    p = _encoder_params(rng, 25, 4)
    lstm = torch.nn.LSTM(D, H, batch_first=True).cuda()
    with torch.no_grad():
        lstm.weight_ih_l0.copy_(_t(p["wx"]).t())
        lstm.weight_hh_l0.copy_(_t(p["wh"]).t())
        lstm.bias_ih_l0.copy_(_t(p["bias"]))
        lstm.bias_hh_l0.zero_()
        _, (hn, _) = lstm(_t(x).flip(1))
        ours = ops.seq_lstm(_t(x), _t(p["wx"]), _t(p["wh"]), _t(p["bias"]), "sigmoid")
    _report("sigmoid LSTM vs torch.nn.LSTM", {"h": rel_err(_np(ours), _np(hn[0]))}, TOL)


def _sample_batch(dev="cuda"):
    import torch
    from kgcn_amd import data_util as D
    g = np.load(GOLDEN)
    channels, _ = D.build_adjs({"dense_adj": g["dense_adj"], "max_node_num": int(g["max_node_num"])})
    tokens, S = D.sequence_table({"sequence": g["sequence"], "sequence_symbol_num": g["sequence_symbol_num"]}, dev)
    dataset = D.DeviceGraphDataset(channels, g["feature"], device=dev)
    return g, channels, dataset, tokens, S


def _model_params_np(model):
    p = {"conv_w": [_np(w) for w in model.conv.w], "conv_b": [_np(b).reshape(-1) for b in model.conv.bias],
         "dense_w": _np(model.dense.kernel), "dense_b": _np(model.dense.bias), "embeddings": _np(model.sequence.embeddings),
         "conv_kernel": _np(model.sequence.conv_kernel), "conv_bias": _np(model.sequence.conv_bias),
         "kernel": _np(model.sequence.kernel), "recurrent_kernel": _np(model.sequence.recurrent_kernel),
         "bias": _np(model.sequence.bias), "hidden_w": _np(model.hidden.kernel), "hidden_b": _np(model.hidden.bias),
         "out_w": _np(model.out.kernel), "out_b": _np(model.out.bias)}
    grads = {"conv_w": [_np(w.grad) for w in model.conv.w], "conv_b": [_np(b.grad).reshape(-1) for b in model.conv.bias],
             "dense_w": model.dense.kernel, "dense_b": model.dense.bias, "embeddings": model.sequence.embeddings,
             "conv_kernel": model.sequence.conv_kernel, "conv_bias": model.sequence.conv_bias, "kernel": model.sequence.kernel,
             "recurrent_kernel": model.sequence.recurrent_kernel, "bias": model.sequence.bias, "hidden_w": model.hidden.kernel,
             "hidden_b": model.hidden.bias, "out_w": model.out.kernel, "out_b": model.out.bias}
    grads = {k: (v if isinstance(v, list) else _np(v.grad)) for k, v in grads.items()}
    return p, grads


def _adjs_list(channels, idx, N):
    out = []
    for b in idx:
        row = []
        for c in channels:
            if b < 0:
                row.append((np.zeros((0, 2), np.int64), np.zeros(0), [N, N]))
            else:
                sel = c.graph == b
                row.append((np.stack([c.row[sel], c.col[sel]], 1), c.val[sel].astype(np.float64), [N, N]))
        out.append(row)
    return out


def _check_model(model, features, adj, tok, labels, mask, adjs_np, tag, act="hard_sigmoid"):
    import torch
    from kgcn_amd import models
    model.zero_grad(set_to_none=True)
    logits = model(features, adj, sequences=tok)
    cost_opt, cost_sum = models.MultimodalGCN.loss(logits, labels, mask)
    cost_opt.backward()
    torch.cuda.synchronize()
    p, grads = _model_params_np(model)
    rl, rc, rs, cache = M.model_fwd(p, _np(features), adjs_np, tok.cpu().numpy(), _np(labels), _np(mask), act)
    rg = M.model_bwd(p, cache)
    errs = {"logits": rel_err(_np(logits), rl), "cost_opt": rel_err(float(cost_opt.detach()), rc), "cost_sum": rel_err(float(cost_sum.detach()), rs)}
    for k in M.PARAM_NAMES:
        if isinstance(rg[k], list):
            errs["d_" + k] = max(rel_err(a, b) for a, b in zip(grads[k], rg[k]))
        else:
            errs["d_" + k] = rel_err(grads[k], rg[k])
    _report(tag, errs, TOL)


def test_model_on_sample_jbl_with_dummy_tail():
    import torch
    from kgcn_amd import models
    g, channels, dataset, tokens, S = _sample_batch()
    B = 10
    sb = dataset.static_batch(B)
    tok = sb.add_table(tokens)
    labels = sb.add_table(_t(g["label"]))
    mask = sb.add_table(torch.ones(dataset.num_graphs, device="cuda"))
    sb.load(np.arange(5))
    assert np.array_equal(tok.cpu().numpy(), g["feed_sequences"][0])       # the reference feed, dummy rows included
    torch.manual_seed(0)
    model = models.MultimodalGCN(S, embedding_dim=4, adj_channel_num=len(channels), label_dim=2).cuda()
    model(sb.features, sb.adjacency, sequences=tok)                        # Keras-style lazy build
    _check_model(model, sb.features, sb.adjacency, tok, labels, mask, _adjs_list(channels, [0, 1, 2, 3, 4] + [-1] * 5, 3),
                 "sample.jbl batch 10")


def _cpi_batch(B=4096, N=50, F=81, L=700, S=25, seed=0):
    import torch
    from oracle import kgcn_oracle as K
    rng = np.random.default_rng(seed)
    adjs = K.synth_mol_graphs(rng, B, N, 1)
    x = rng.standard_normal((B, N, F)).astype(np.float32) * 0.3
    tok = rng.integers(0, S, size=(B, L)).astype(np.int32)
    lens = rng.integers(L // 4, L + 1, size=B)
    tok[np.arange(L)[None, :] >= lens[:, None]] = 0
    lab = np.eye(2)[rng.integers(0, 2, size=B)]
    return adjs, x, torch.as_tensor(tok, device="cuda"), lab


def test_model_at_cpi_shape_against_oracle():
    import torch
    from kgcn_amd import models
    B = 512
    adjs, x, tok, lab = _cpi_batch(B=B)
    torch.manual_seed(1)
    model = models.MultimodalGCN(25, embedding_dim=25, label_dim=2).cuda()
    feats = _t(x)
    model(feats, adjs, sequences=tok)
    mask = torch.ones(B, device="cuda")
    mask[-3:] = 0
    _check_model(model, feats, adjs, tok, _t(lab), mask, adjs, "CPI shape, 512 pairs, 50 atoms, L = 700, E = 25")


def _setup_training(S_dev=None):
    import torch
    from kgcn_amd import models, train
    g, channels, dataset, tokens, S = _sample_batch()
    torch.manual_seed(0)
    model = models.MultimodalGCN(S, embedding_dim=4, adj_channel_num=len(channels), label_dim=2).cuda()
    sb = dataset.static_batch(10)
    tok = sb.add_table(tokens)
    labels = sb.add_table(_t(g["label"]))
    mask = sb.add_table(torch.ones(dataset.num_graphs, device="cuda"))
    sb.load(np.arange(5))
    model(sb.features, sb.adjacency, sequences=tok)
    opt = train.TFAdam(model.parameters(), lr=0.3)
    return model, opt, sb, tok, labels, mask


def test_two_runs_bit_identical():
    import torch
    from kgcn_amd import models, ops
    adjs, x, tok, lab = _cpi_batch(B=1024, seed=4)
    outs = []
    for _ in range(2):
        torch.manual_seed(2)
        model = models.MultimodalGCN(25, embedding_dim=25).cuda()
        feats = _t(x)
        model(feats, adjs, sequences=tok)
        logits = model(feats, adjs, sequences=tok)
        cost, _ = models.MultimodalGCN.loss(logits, _t(lab), torch.ones(1024, device="cuda"))
        with ops.deferred_reductions(root=cost):
            cost.backward()
        torch.cuda.synchronize()
        outs.append([_np(logits)] + [_np(q.grad) for q in model.parameters()])
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_replays_equal_eager_steps():
    import torch
    from kgcn_amd import models, train
    k = 4
    model, opt, sb, tok, labels, mask = _setup_training()
    p0 = [q.detach().clone() for q in model.parameters()]
    eager = []
    for _ in range(k):
        cs, _ = train.train_step(model, opt, models.MultimodalGCN.loss, sb.features, sb.adjacency, labels, mask, sequences=tok)
        eager.append(cs)
    p_eager = [_np(q) for q in model.parameters()]
    with torch.no_grad():
        for q, q0 in zip(model.parameters(), p0):
            q.copy_(q0)
    model2, opt2 = model, train.TFAdam(model.parameters(), lr=0.3)
    step = train.GraphedTrainStep(model2, opt2, models.MultimodalGCN.loss, sb, labels, mask, capture_assembly=True, sequences=tok)
    replayed = []
    for _ in range(k):
        sb.stage(np.arange(5))
        cs, _ = step.replay()
        replayed.append(float(cs))
    torch.cuda.synchronize()
    assert replayed == eager, (replayed, eager)
    for a, b in zip(p_eager, [_np(q) for q in model.parameters()]):
        assert np.array_equal(a, b)
    assert len(set(eager)) == k                      # every step moved the parameters


def test_no_torch_operator_inside_the_captured_step():
    from kgcn_amd import models, train
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from aten_in_step import log_step
    model, opt, sb, tok, labels, mask = _setup_training()
    step = train.GraphedTrainStep(model, opt, models.MultimodalGCN.loss, sb, labels, mask, capture_assembly=True, sequences=tok)
    seen = log_step(step._eager)
    assert not seen, dict(seen)


def test_limits_raise_on_the_device_path():
    import torch
    from kgcn_amd import _lib, ops
    tok = torch.zeros((2, 16), dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.KgcnHipError):
        ops.seq_conv_pool(tok, torch.zeros((25, 33), device="cuda"), torch.zeros((4, 33, 50), device="cuda"),
                          torch.zeros(50, device="cuda"), 4)
    with pytest.raises(_lib.KgcnHipError):
        ops.seq_lstm(torch.zeros((2, 4, 50), device="cuda"), torch.zeros((50, 260), device="cuda"),
                     torch.zeros((65, 260), device="cuda"), torch.zeros(260, device="cuda"))
