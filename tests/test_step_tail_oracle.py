"""CPU checks of tests/step_tail_oracle.py, the fp64 reference the loss heads and the TF-Adam kernels are compared with
(tests/test_gpu_loss_heads.py, tests/test_gpu_adam_forms.py):
  - against the oracles the project already trusts (oracle/kgcn_nets_oracle.py, oracle/kgcn_model_oracle.py) at 1e-12;
  - every gradient against central differences;
  - on the very inputs of the GPU tests (tests/step_tail_cases.py): a head or an update that is wrong in one of five likely ways
    lands at least TEN times outside the bound the GPU tests assert, so those tests would notice such a kernel.  Numpy alone: no
    kernel and no product code is altered to show it.
"""
import numpy as np
import pytest

import step_tail_cases as C
import step_tail_oracle as R
from conftest import load_golden, unflatten_adjs
from oracle import kgcn_model_oracle as M
from oracle import kgcn_nets_oracle as NETS

AGREE = 1e-12


def _close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    err = float(np.abs(a - b).max()) if a.size else 0.0
    assert err <= AGREE * max(1.0, float(np.abs(b).max()) if b.size else 0.0), (what, err)


# ---- against the trusted oracles ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [2, 257])
def test_sigmoid_head_agrees_with_the_multitask_oracle(B):
    """oracle.kgcn_nets_oracle.sigmoid_ce / sigmoid_ce_grad (the loss lines of multitask_forward / multitask_backward, :78-88) on
    every sigmoid case of the GPU test at this batch size -- saturated logits, scalar and per-task weights included."""
    for d in C.sigmoid_cases(B):
        x, z = d["logits"].astype(np.float64), d["labels"].astype(np.float64)
        ml = np.ones_like(x) if d["mask_label"] is None else d["mask_label"].astype(np.float64)
        mk = d["mask"].astype(np.float64)
        pw = None if d["pos_weight"] is None else np.asarray(d["pos_weight"], np.float64)
        cost = mk * (ml * NETS.sigmoid_ce(x, z, pw)).sum(axis=1)
        dl = mk[:, None] * ml * NETS.sigmoid_ce_grad(x, z, pw)
        got = R.sigmoid_ce(d["logits"], d["labels"], d["mask"], d["mask_label"], d["pos_weight"])
        tag = (d["T"], d["weights"], d["label_mask"], d["mask_kind"], d["regime"])
        _close(got[0], cost, ("cost",) + tag)
        _close(got[1], dl, ("dlogits",) + tag)
        _close(got[2], cost.sum(), ("cost_sum",) + tag)
        _close(got[3], cost.mean(), ("cost_opt",) + tag)


@pytest.mark.parametrize("labels", ["golden", "soft_scaled"])
def test_softmax_head_agrees_with_the_model_oracle(labels):
    """The loss lines of oracle.kgcn_model_oracle.forward (:48-51) and backward (:58-60) on the logits of the model itself:
    cost_opt, cost_sum, and d cost_opt / d logits seen through the output layer's gradients g["ob"] and g["ok"]."""
    z = load_golden("g3_synthetic_feed_full30.npz")
    x, adjs, mask = z["features"].astype(np.float64), unflatten_adjs(z, "adj_"), z["mask"].astype(np.float64)
    lab = z["labels"].astype(np.float64)
    if labels == "soft_scaled":
        lab = C.soft_labels("soft_scaled", lab.shape[0], lab.shape[1], np.random.default_rng(3)).astype(np.float64)
        mask = C.graph_mask("tail", lab.shape[0]).astype(np.float64)
    p = M.init_params(np.random.default_rng(0), 3)
    c = M.forward(p, x, adjs, lab, mask)
    g = M.backward(p, c, x, adjs, lab, mask)
    cost, dl, cost_sum, cost_opt = R.softmax_ce(c["logits"], lab, mask)
    _close(cost_sum, c["cost_sum"], "cost_sum")
    _close(cost_opt, c["cost_opt"], "cost_opt")
    dlogits = R.loss_grad(dl, 1.0, None, lab.shape[0])
    _close(dlogits.sum(axis=0), g["ob"], "d ob")
    _close(c["pool"].T @ dlogits, g["ok"], "d ok")
    if labels == "golden":                        # one-hot: the sparse head is the same function of the class index
        sp = R.sparse_softmax_ce(c["logits"], lab.argmax(axis=1), mask)
        _close(sp[0], cost, "sparse cost")
        _close(sp[1], dl, "sparse dlogits")


def test_tf_adam_agrees_with_the_model_oracle():
    """oracle.kgcn_model_oracle.TFAdam over three steps.  The hyper-parameters are exact in float32 (2^-7, 7/8, 1 - 2^-8, 2^-27), so
    the rounding R.tf_adam applies to them changes nothing and the two must agree to 1e-12; with the decimal 0.9 they would not:
    float32(0.9) = 0.9 + 2.4e-8 and 1.0f - float32(0.9) = 0.1 - 2.4e-8."""
    hyper = dict(lr=2.0 ** -7, b1=0.875, b2=1 - 2.0 ** -8, eps=2.0 ** -27)
    rng = np.random.default_rng(5)
    p = {"w": rng.standard_normal((6, 5))}
    opt = M.TFAdam(lr=hyper["lr"], b1=hyper["b1"], b2=hyper["b2"], eps=hyper["eps"])
    q, m, v = p["w"].copy(), np.zeros((6, 5)), np.zeros((6, 5))
    for t in range(1, 4):
        g = rng.standard_normal((6, 5)) * 10.0 ** rng.uniform(-6, 2, (6, 5))
        p = opt.step(p, {"w": g})
        q, m, v = R.tf_adam(q, g, m, v, t, **hyper)
        _close(q, p["w"], ("p", t))
        _close(m, opt.m["w"], ("m", t))
        _close(v, opt.v["w"], ("v", t))
    lr, b1, b2, eps, c1, c2 = R.adam_hyper(1e-2, 0.9, 0.999, 1e-8)
    assert b1 == float(np.float32(0.9)) and c1 == float(np.float32(1) - np.float32(0.9))
    assert 1e-8 < abs(c1 - 0.1) / 0.1 < 1e-6 and abs(b1 + c1 - 1.0) < 1e-15


# ---- gradients against central differences -------------------------------------------------------------------------------------
def _central(f, x, h=1e-5):
    g = np.zeros_like(x)
    flat, gf = x.reshape(-1), g.reshape(-1)
    for i in range(flat.size):
        keep = flat[i]
        flat[i] = keep + h
        up = f(x)
        flat[i] = keep - h
        gf[i] = (up - f(x)) / (2 * h)
        flat[i] = keep
    return g


def _fd_inputs(W, seed):
    rng = np.random.default_rng(seed)
    B = 6
    return rng, B, rng.standard_normal((B, W)) * 2, np.array([1, 1, 0, 1, 1, 0], np.float64)


@pytest.mark.parametrize("weights", C.SIGMOID_WEIGHTS)
def test_sigmoid_gradient_by_central_differences(weights):
    """h = 1e-5 in fp64: truncation h^2 f''' / 6 ~ 1e-10 and rounding eps |f| / h ~ 1e-9 for a cost_sum of order 100; 1e-7 of
    max(1, |gradient|) is a hundred times both."""
    rng, B, x, mask = _fd_inputs(4, 1)
    z = (rng.random((B, 4)) < 0.4).astype(np.float64)
    ml = (rng.random((B, 4)) < 0.8).astype(np.float64)
    pw = {"off": None, "scalar": 2.5, "per_task": np.geomspace(0.2, 40, 4)}[weights]
    for mask_label in (None, ml):
        dl = R.sigmoid_ce(x, z, mask, mask_label, pw)[1]
        num = _central(lambda a: R.sigmoid_ce(a, z, mask, mask_label, pw)[2], x.copy())
        assert np.abs(num - dl).max() <= 1e-7 * max(1.0, np.abs(dl).max())
        assert np.all(dl[mask == 0] == 0)
    # a / b of (a cost_opt + b cost_sum) through loss_grad
    for a, b in C.AUTOGRAD_UPSTREAM:
        f = lambda v: (lambda r: a * r[3] + b * r[2])(R.sigmoid_ce(v, z, mask, ml, pw))
        want = R.loss_grad(R.sigmoid_ce(x, z, mask, ml, pw)[1], a if a else None, b if b else None, B)
        num = _central(f, x.copy())
        assert np.abs(num - want).max() <= 1e-7 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("labels", C.SOFTMAX_LABELS)
def test_softmax_gradient_by_central_differences(labels):
    rng, B, x, mask = _fd_inputs(5, 2)
    z = C.soft_labels(labels, B, 5, rng).astype(np.float64)
    dl = R.softmax_ce(x, z, mask)[1]
    num = _central(lambda a: R.softmax_ce(a, z, mask)[2], x.copy())
    assert np.abs(num - dl).max() <= 1e-7 * max(1.0, np.abs(dl).max())
    for a, b in C.AUTOGRAD_UPSTREAM:
        f = lambda v: (lambda r: a * r[3] + b * r[2])(R.softmax_ce(v, z, mask))
        want = R.loss_grad(dl, a if a else None, b if b else None, B)
        assert np.abs(_central(f, x.copy()) - want).max() <= 1e-7 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("masked", [False, True])
def test_sparse_softmax_gradient_by_central_differences(masked):
    rng, B, x, mask = _fd_inputs(5, 3)
    idx = np.array([0, 4, 2, 2, 1, 3])
    mk = mask if masked else None
    dl = R.sparse_softmax_ce(x, idx, mk)[1]
    num = _central(lambda a: R.sparse_softmax_ce(a, idx, mk)[2], x.copy())
    assert np.abs(num - dl).max() <= 1e-7 * max(1.0, np.abs(dl).max())
    want = R.loss_grad(dl, None, 3.0, 1)
    num3 = _central(lambda a: 3.0 * R.sparse_softmax_ce(a, idx, mk)[2], x.copy())
    assert np.abs(num3 - want).max() <= 1e-7 * max(1.0, np.abs(want).max())


# ---- the GPU tests' own inputs: properties they rely on, and what a wrong kernel would show on them -----------------------------
def _array_bound(ref):
    return C.ARRAY_TOL * max(1.0, float(np.abs(ref).max()))


@pytest.mark.parametrize("B", C.BATCHES)
def test_cost_sums_of_the_gpu_cases_are_zero_or_of_order_one(B):
    """The GPU tests hold sums[0] / sums[1] to 1e-6 RELATIVE.  That asks something of float32 only while the sum is made of terms
    float32 can carry: a batch whose whole cost is log(1 + exp(-120)) = 8e-53 has no float32 value but 0.  Every case's cost_sum
    is therefore either exactly 0 (nothing live) or at least 1e-3 -- the saturated logits of the grid always sit beside terms of
    order one -- and no cost is negative, so the sum never cancels."""
    refs = [R.sigmoid_ce(d["logits"], d["labels"], d["mask"], d["mask_label"], d["pos_weight"]) for d in C.sigmoid_cases(B)]
    refs += [R.softmax_ce(d["logits"], d["labels"], d["mask"]) for d in C.softmax_cases(B)]
    refs += [R.sparse_softmax_ce(d["logits"], d["idx"], d["mask"]) for d in C.sparse_cases(B)]
    for cost, dl, s, mean in refs:
        assert np.all(cost >= 0) and np.all(np.isfinite(dl))
        assert s == 0.0 or s >= 1e-3, s


@pytest.mark.parametrize("B", C.BATCHES)
def test_wrong_mean_over_the_unmasked_count_is_seen(B):
    """cost_opt = cost_sum / (number of live graphs) instead of / B (quirk Q5): on every GPU case whose mask has a dummy row beside
    a live one, the wrong sums[1] is off by at least 10 x the 1e-6 relative bound."""
    seen = 0
    for d, r in [(d, R.sigmoid_ce(d["logits"], d["labels"], d["mask"], d["mask_label"], d["pos_weight"])) for d in C.sigmoid_cases(B)] + \
                [(d, R.softmax_ce(d["logits"], d["labels"], d["mask"])) for d in C.softmax_cases(B)] + \
                [(d, R.sparse_softmax_ce(d["logits"], d["idx"], d["mask"])) for d in C.sparse_cases(B)]:
        mk = d["mask"]
        if mk is None or not (0 < mk.sum() < B) or r[2] == 0.0:
            continue
        wrong = r[2] / float(mk.sum())
        assert abs(wrong - r[3]) >= 10 * C.SUM_TOL * abs(r[3])
        seen += 1
    assert seen > 0 or B == 1                     # B = 1 has no room for a dummy beside a live graph


@pytest.mark.parametrize("B", C.BATCHES)
def test_wrong_softmax_gradient_without_the_label_sum_is_seen(B):
    """d cost / d x = softmax - z instead of softmax * sum_c z - z: on every GPU case with live rows whose labels do not sum to 1
    (soft_scaled: 0.3 and 2; zero_rows: 0), the wrong dlogits are off by at least 10 x the array bound."""
    seen = 0
    for d in C.softmax_cases(B):
        if d["label_kind"] not in ("soft_scaled", "zero_rows") or d["mask_kind"] == "zero":
            continue
        x, z, mk = d["logits"].astype(np.float64), d["labels"].astype(np.float64), d["mask"].astype(np.float64)
        s = x - x.max(axis=1, keepdims=True)
        soft = np.exp(s) / np.exp(s).sum(axis=1, keepdims=True)
        wrong = mk[:, None] * (soft - z)
        ref = R.softmax_ce(x, z, mk)[1]
        assert np.abs(wrong - ref).max() >= 10 * _array_bound(ref), (d["C"], d["label_kind"], d["regime"])
        seen += 1
    assert seen > 0


@pytest.mark.parametrize("B", [b for b in C.BATCHES if b >= 255])
def test_wrong_pos_weight_by_row_is_seen(B):
    """The per-task weight read by ROW (q[b mod T]) instead of by COLUMN (q[t]): on every GPU case with a per-task vector of more
    than one task and live rows, cost and dlogits are both off by at least 10 x the array bound.  (At B <= 2 a single live row
    may carry no positive label outside column 0, where the two readings agree; from B = 255 on that cannot happen.)"""
    seen = 0
    for d in C.sigmoid_cases(B):
        if d["weights"] != "per_task" or d["T"] == 1 or d["mask_kind"] == "zero":
            continue
        by_row = d["qvec"][np.arange(B) % d["T"]].astype(np.float64)[:, None] * np.ones((1, d["T"]))
        ref = R.sigmoid_ce(d["logits"], d["labels"], d["mask"], d["mask_label"], d["qvec"])
        # the same formulas with a full [B, T] weight table in place of the per-column vector
        x, z = d["logits"].astype(np.float64), d["labels"].astype(np.float64)
        ml = np.ones_like(x) if d["mask_label"] is None else d["mask_label"].astype(np.float64)
        mk = d["mask"].astype(np.float64)
        cost = mk * (ml * NETS.sigmoid_ce(x, z, by_row)).sum(axis=1)
        dl = mk[:, None] * ml * NETS.sigmoid_ce_grad(x, z, by_row)
        tag = (d["T"], d["label_mask"], d["regime"])
        assert np.abs(cost - ref[0]).max() >= 10 * _array_bound(ref[0]), tag
        assert np.abs(dl - ref[1]).max() >= 10 * _array_bound(ref[1]), tag
        seen += 1
    assert seen > 0


@pytest.mark.parametrize("regime", ["normal", "grid"])
def test_wrong_upstream_gradient_not_divided_by_the_batch_is_seen(regime):
    """d logits = dlogits (g_sum + g_opt) instead of dlogits (g_sum + g_opt / B) on the inputs of the autograd tests, for both
    upstream pairs that have a g_opt: off by at least 10 x the array bound."""
    ds, dm = C.autograd_sigmoid_case(regime), C.autograd_softmax_case(regime)
    for dl in (R.sigmoid_ce(ds["logits"], ds["labels"], ds["mask"], ds["mask_label"], ds["pos_weight"])[1],
               R.softmax_ce(dm["logits"], dm["labels"], dm["mask"])[1]):
        for a, b in C.AUTOGRAD_UPSTREAM:
            if a == 0.0:
                continue
            ref = R.loss_grad(dl, a, b if b else None, C.AUTOGRAD_B)
            wrong = dl * (a + b)
            assert np.abs(wrong - ref).max() >= 10 * _array_bound(ref)


@pytest.mark.parametrize("counter", C.ADAM_COUNTERS)
@pytest.mark.parametrize("n", C.ADAM_SIZES)
def test_wrong_adam_epsilon_inside_the_root_is_seen(n, counter):
    """p -= lr_t m / sqrt(v + eps) instead of lr_t m / (sqrt(v) + eps): on every (size, counter) case of the GPU test, after each of
    the three steps some parameter is off by at least 10 x (2e-6 + 2e-6 |reference|)."""
    d = C.adam_case(n, counter)
    lr_, b1_, b2_, eps_, c1, c2 = R.adam_hyper(**C.ADAM_HYPER)
    p = d["p"].astype(np.float64)
    m, v = d["m"].astype(np.float64), d["v"].astype(np.float64)
    pw, mw, vw = p.copy(), m.copy(), v.copy()
    for k, g in enumerate(d["grads"]):
        t = counter + 1 + k
        p, m, v = R.tf_adam(p, g, m, v, t, **C.ADAM_HYPER)
        g64 = g.astype(np.float64)
        mw = b1_ * mw + c1 * g64
        vw = b2_ * vw + c2 * g64 * g64
        pw = pw - R.adam_lr_t(t, C.ADAM_HYPER["lr"], C.ADAM_HYPER["b1"], C.ADAM_HYPER["b2"]) * mw / np.sqrt(vw + eps_)
        assert np.all(np.isfinite(p)) and np.all(v >= 0)
        assert (np.abs(pw - p) - 10 * (C.ADAM_ATOL + C.ADAM_RTOL * np.abs(p))).max() >= 0, (n, counter, k)


def test_adam_segments_cover_the_buffer_with_an_empty_one():
    for n in C.ADAM_SIZES:
        for k in C.ADAM_SEGMENT_COUNTS:
            segs = C.adam_segments(n, k)
            assert len(segs) == k and segs[0][0] == 0 and sum(l for _, l in segs) == n
            assert all(segs[i][0] + segs[i][1] == segs[i + 1][0] for i in range(k - 1))
            assert k < 3 or any(l == 0 for _, l in segs)
