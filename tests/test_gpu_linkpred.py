"""Knowledge-graph link prediction on the GPU (csrc/linkpred.hip, ops.linkpred_loss, models.LinkPredictionNet) against the fp64
oracle of tests/linkpred_oracle.py: the device negative draw, the loss and its gradients, the whole training step on the BA
fixture, and the captured step's determinism."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import linkpred_oracle as O  # noqa: E402
from gpu_helpers import to_device as _t, to_f64 as _np  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-5
MODES = ("gcn", "distmult", "ip")
GOLDEN = os.path.join(ROOT, "tests", "golden", "g8_kg_linkpred.npz")
LR = {"gcn": 0.001, "distmult": 0.01, "ip": 0.001}


def _i(a):
    return _t(a, np.int32)


def err(a, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / max(1.0, np.abs(ref).max()))


def _feed(lab, L, device="cuda"):
    from kgcn_amd import data_util as D
    return D.LinkPredFeed(lab, batch=L, device=device)


# ---- negative draw ---------------------------------------------------------------------------------------------------------
def test_device_negatives_and_rows_equal_the_host_restatement():
    import torch
    from kgcn_amd import ops
    rng = np.random.default_rng(0)
    N, M, L = 300, 70, 7
    lab = np.stack([rng.integers(0, N, M), rng.integers(0, 3, M), rng.integers(0, N, M), rng.integers(0, N, M),
                    np.zeros(M, np.int64), rng.integers(0, N, M)], 1)
    feed = _feed(lab, L)
    perm = feed.shuffle(np.random.RandomState(5)).copy()
    h = _t(rng.standard_normal((N, 16)))
    step = torch.zeros((), dtype=torch.int64, device="cuda")
    for s in (0, 3, 12, 2 ** 40 + 7):
        step.fill_(s)
        *_, rows = ops.linkpred_loss(h, feed, "gcn", seed=123, step=step)
        ref = O.assemble(lab, perm, _all_label(lab), L, 123, s)
        assert np.array_equal(rows.cpu().numpy(), ref), s


def _all_label(lab):
    return np.unique(np.concatenate([lab[:, 0], lab[:, 2]]))


# ---- loss and gradients -------------------------------------------------------------------------------------------------
def _loss_case(mode, L, hub=False, overflow=False, seed=0):
    rng = np.random.default_rng(seed + L)
    N, D, R = 2000, 128, 3
    M = 2 * L
    lab = np.stack([rng.integers(0, N, M), rng.integers(0, R, M), rng.integers(0, N, M), rng.integers(0, N, M),
                    rng.integers(0, R, M), rng.integers(0, N, M)], 1)
    if hub:                                        # node 5 in more than half of the rows (cols 0 and 3 after assembly)
        lab[rng.random(M) < 0.7, 0] = 5
    h = rng.standard_normal((N, D)) * 0.3
    w = rng.standard_normal((R, D)) * 0.5
    if overflow:                                   # rows whose s2 - s1 leaves fp32's exp range
        w = np.abs(w)
        h[7] = 10.0
        h[N - 1] = -10.0
        lab[L:L + L // 2 + 1, 0] = 7                # window 1 (step 1 of two windows)
        lab[L:L + L // 2 + 1, 2] = N - 1
    return lab, np.float32(h), np.float32(w)


def _run_loss(mode, lab, h, w, L, g_opt=1.0, g_sum=0.25, seed=77, step_val=1):
    import torch
    from kgcn_amd import ops
    feed = _feed(lab, L)
    th = _t(h).requires_grad_(True)
    tw = _t(w).requires_grad_(True) if mode == "distmult" else None
    step = torch.tensor(step_val, dtype=torch.int64, device="cuda")
    c_opt, c_sum, correct, s1, s2, rows = ops.linkpred_loss(th, feed, mode, w=tw, seed=seed, step=step)
    torch.autograd.backward([c_opt, c_sum], [torch.tensor(g_opt, device="cuda"), torch.tensor(g_sum, device="cuda")])
    torch.cuda.synchronize()
    return c_opt, c_sum, correct, s1, s2, rows.cpu().numpy().astype(np.int64), th.grad, (tw.grad if tw is not None else None)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("L,hub,overflow", [(1, False, False), (7, False, False), (1000, False, False), (4096, False, False),
                                            (1000, True, False), (64, False, True)])
def test_loss_and_gradients_against_oracle(mode, L, hub, overflow):
    lab, h, w = _loss_case(mode, L, hub, overflow)
    c_opt, c_sum, correct, s1, s2, rows, dh, dw = _run_loss(mode, lab, h, w, L)
    ref_rows = O.assemble(lab, None, _all_label(lab), L, 77, 1)
    assert np.array_equal(rows, ref_rows)
    ww = w if mode == "distmult" else None
    r1, r2 = O.scores(h, rows, mode, ww)
    res = O.loss(r1, r2, mode)
    assert err(_np(s1), r1) < TOL and err(_np(s2), r2) < TOL
    c_opt, c_sum = float(c_opt.detach()), float(c_sum.detach())
    assert err(c_opt, res["cost_opt"]) < TOL, (c_opt, res["cost_opt"])
    assert err(c_sum, res["cost_sum"]) < TOL
    if mode != "ip":
        # a comparison within fp32 rounding of a tie may flip
        ties = int((np.abs(r1 - r2) < 1e-5 * np.maximum(1.0, np.abs(r1))).sum())
        assert abs(float(correct) - res["correct_count"]) <= ties
    gh, gw = O.loss_grads(h, rows, mode, ww, 1.0, 0.25)
    assert np.isfinite(_np(dh)).all()
    assert err(_np(dh), gh) < TOL, err(_np(dh), gh)
    if mode == "distmult":
        assert err(_np(dw), gw) < TOL, err(_np(dw), gw)
    if overflow and mode != "ip":
        x = r2 - r1 + 0.1
        assert (x > 89).any()                      # the case really leaves the exp range


def test_loss_bitwise_reproducible_under_skew():
    lab, h, w = _loss_case("distmult", 4096, hub=True)
    a = _run_loss("distmult", lab, h, w, 4096)
    b = _run_loss("distmult", lab, h, w, 4096)
    assert np.array_equal(_np(a[6]), _np(b[6])) and np.array_equal(_np(a[7]), _np(b[7]))
    assert float(a[0].detach()) == float(b[0].detach())


# ---- whole model on the fixture -------------------------------------------------------------------------------------------
def _fixture():
    from kgcn_amd import data_util as D
    z = np.load(GOLDEN)
    data = {"adj": [(z["adj_idx"], z["adj_val"], np.array([int(z["node_num"])] * 2))], "node": z["node"],
            "node_num": z["node_num"], "label_list": z["label_list"], "test_label_list": z["test_label_list"]}
    return D.LinkPredictionData(data), z


def _setup(mode, seed=0):
    import torch
    from kgcn_amd import data_util as D, models, train
    data, z = _fixture()
    train_list, _ = D.split_label_list(data.label_list, 0.2, np.random.RandomState(seed))
    adj = data.adjacency() if mode == "gcn" else None
    feed = D.LinkPredFeed(train_list, batch=1000, adjacency=adj)
    torch.manual_seed(seed)
    model = models.LinkPredictionNet(mode, data.num_nodes, data.num_relations, seed=99, device="cuda")
    model(None, adj, feed=feed)                  # builds the GraphConv parameters
    opt = train.TFAdam(model.parameters(), lr=LR[mode])
    model.bind_step(opt._t_dev)
    return data, z, feed, adj, model, opt


def _params(model):
    p = {"embedding": _np(model.embedding)}
    if model.variant == "gcn":
        p.update(w1=_np(model.conv1.w[0]), b1=_np(model.conv1.bias[0]).reshape(-1), w2=_np(model.conv2.w[0]),
                 b2=_np(model.conv2.bias[0]).reshape(-1))
    if model.distmult is not None:
        p["w"] = _np(model.distmult.w[0])
    return p


def _tensors(model):
    t = {"embedding": model.embedding}
    if model.variant == "gcn":
        t.update(w1=model.conv1.w[0], b1=model.conv1.bias[0], w2=model.conv2.w[0], b2=model.conv2.bias[0])
    if model.distmult is not None:
        t["w"] = model.distmult.w[0]
    return t


@pytest.mark.parametrize("mode", MODES)
def test_whole_step_against_oracle(mode):
    import torch
    from kgcn_amd import train
    data, z, feed, adj, model, opt = _setup(mode)
    p0 = _params(model)
    cs, _ = train.train_step(model, opt, model.loss, None, adj, None, None, feed=feed)
    torch.cuda.synchronize()
    rows = model.rows.cpu().numpy().astype(np.int64)
    assert np.array_equal(rows, O.assemble(feed.label_list, None, _all_label(feed.label_list), 1000, 99, 0))
    A = O.dense_adj(z["adj_idx"], z["adj_val"], data.num_nodes) if mode == "gcn" else None
    res, g = O.model_grads(p0, mode, rows, A)
    assert err(cs, res["cost_sum"]) < TOL, (cs, res["cost_sum"])
    for name, t in _tensors(model).items():
        gg = g[name].reshape(t.shape)
        assert err(_np(t.grad), gg) < TOL, (name, err(_np(t.grad), gg))
        # the update itself, from the gradient the step produced (checked just above): where |g| is near Adam's eps a relative
        # gradient error of 1e-5 would move the step by a visible fraction of lr
        pn, _, _ = O.tf_adam(p0[name].reshape(t.shape), _np(t.grad), 0.0, 0.0, 1, LR[mode])
        assert err(_np(t), pn) < 1e-6, (name, err(_np(t), pn))


# ---- captured step ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_replay_equals_eager_and_replays_repeat(mode):
    import torch
    from kgcn_amd import train
    k = 4
    data, z, feed, adj, model, opt = _setup(mode)
    eager = [train.train_step(model, opt, model.loss, None, adj, None, None, feed=feed)[0] for _ in range(k)]
    p_eager = [_np(q) for q in model.parameters()]
    data, z, feed, adj, model, opt = _setup(mode)
    step = train.GraphedTrainStep(model, opt, model.loss, feed, None, None, feed=feed)
    replayed = [float(step.replay()[0]) for _ in range(k)]
    torch.cuda.synchronize()
    assert replayed == eager, (replayed, eager)
    for a, b in zip(p_eager, [_np(q) for q in model.parameters()]):
        assert np.array_equal(a, b)
    # 20 replays from the same state agree bit for bit
    saved = [q.detach().clone() for q in list(opt.params) + opt.m + opt.v]
    t0 = opt.t
    outs = []
    for _ in range(20):
        with torch.no_grad():
            for dst, src in zip(list(opt.params) + opt.m + opt.v, saved):
                dst.copy_(src)
            opt._t_dev.fill_(t0)
        opt.t = t0
        cs, _ = step.replay()
        torch.cuda.synchronize()
        outs.append((float(cs), model.embedding.detach().cpu().numpy().tobytes()))
    assert all(o == outs[0] for o in outs[1:])


@pytest.mark.parametrize("mode", MODES)
def test_no_torch_operator_inside_the_captured_step(mode):
    from kgcn_amd import train
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from aten_in_step import log_step
    data, z, feed, adj, model, opt = _setup(mode)
    step = train.GraphedTrainStep(model, opt, model.loss, feed, None, None, feed=feed)
    seen = log_step(step._eager)
    assert not seen, dict(seen)
