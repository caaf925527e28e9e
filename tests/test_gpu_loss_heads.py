"""The loss heads of csrc/train.hip as OPERATIONS, against the fp64 reference of tests/step_tail_oracle.py on the cases of
tests/step_tail_cases.py: sigmoid_ce_kernel, softmax_ce_kernel (dense and sparse labels), loss_finish_kernel through the C entry
points (the per-graph `cost` output and the sparse head's `mask` exist only there), loss_grad_kernel through the autograd
wrappers of ops.py.

Which gap of the suite each test closes:
  the one-workgroup shortcut (B <= 256: the loss kernel writes the sums) and the finishing launch (B >= 257), the tail lanes of
    the last workgroup                                    every test_*_head[B]: B = 1, 2, 255, 256 | 257, 513, 1025
  the per-graph cost output, and cost = NULL              every test_*_head[B]
  the mask operand of kgcn_sparse_softmax_ce_f32          test_sparse_softmax_head (NULL, padded tail, all zero)
  soft labels, rows that do not sum to 1                  test_softmax_head (soft1, soft_scaled, zero_rows)
  sigmoid: unweighted with mask_label = NULL, per-task weights at widths 1 and 5, logits beyond +-20
                                                          test_sigmoid_head (weights off x label mask none; per_task x T = 1, 5; grid)
  loss_grad_kernel with g_sum alone and with both upstream gradients
                                                          test_autograd_* ((0, 1) and (0.7, -1.3))

Bounds (tests/step_tail_cases.py): cost and dlogits within 2e-6 * max(1, max |reference|) per array, the two sums within 1e-6
relative (1e-6 absolute where the reference is 0).  The largest errors measured on an MI355X, per head and regime, stand beside
those bounds in tests/step_tail_cases.py; every session records them again (conftest.record_accuracy).  No regime needed a
bound of its own: where sigmoid and softplus saturate (|x| >= 20) the kernel's 1 / (1 + __expf(-x)) and
log1pf(__expf(-|x|)) are off by a relative 1e-6 of terms that are themselves below 1e-8.

What these tests found in csrc/train.hip, each corrected there (the cases stay as they were):
  sigmoid head, weighted branch, cost: (1 - z) x + lw (sp + max(-x, 0)) as written cancels for x < 0 -- B = 1, T = 5, scalar
    weight, a row of five logits -5.68 with z = 0: sums[0] 0.01692295 against 0.01692183, 6.6e-5 relative.
  sigmoid head, weighted branch, gradient: (1 - z) - lw (1 - sg) multiplies the rounding of an sg next to 1 by lw <= 40 --
    B = 2, T = 12, per-task weights, N(0, 3): dlogits off by 2.6e-6 of a gradient of order one.
  softmax heads: log(sum exp) of a confident row is log(1.019) with the 0.019 already rounded -- sparse head, B = 1, C = 2,
    N(0, 3): sums[0] 0.01902710 against 0.01902714, 2.1e-6 relative.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import step_tail_cases as C  # noqa: E402
import step_tail_oracle as R  # noqa: E402
from conftest import record_accuracy  # noqa: E402

pytestmark = pytest.mark.gpu

# this session's largest errors: head -> regime -> {cost, dlogits: error / max(1, max |ref|); sums: relative error}; printed per test
_WORST = {}

_GARBAGE = 12345.678          # what the output buffers hold before a call


def dev():
    return torch.device("cuda:0")


def _up(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _bits(t):
    return t.view(torch.int32)


def _run(call, B, W):
    """call(cost, dlogits, sums, ws, ws_bytes) -> rc.  Runs it with a cost buffer and with cost = NULL into fresh buffers, asserts
    the two give the same bytes in dlogits and sums, -> (cost, dlogits, sums) as numpy arrays."""
    from kgcn_amd import _lib
    wsb = int(_lib.lib.kgcn_loss_workspace_bytes(B))
    assert wsb >= 4 * ((B + 255) // 256)
    outs = []
    for with_cost in (True, False):
        cost = torch.full((B,), _GARBAGE, device=dev())
        dl = torch.full((B, W), _GARBAGE, device=dev())
        sums = torch.full((2,), _GARBAGE, device=dev())
        ws = torch.full((max(wsb // 4, 1),), _GARBAGE, device=dev())
        _lib.check(call(cost if with_cost else None, dl, sums, ws, wsb), "loss head")
        outs.append((cost, dl, sums))
    (cost, dl, sums), (untouched, dl2, sums2) = outs
    assert torch.equal(_bits(dl), _bits(dl2)) and torch.equal(_bits(sums), _bits(sums2)), "cost = NULL changed dlogits or sums"
    assert bool((untouched == _GARBAGE).all())
    return cost.cpu().numpy(), dl.cpu().numpy(), sums.cpu().numpy()


def _check(head, d, got, ref, zero_elems=None):
    """The assertions every head shares.  got = (cost, dlogits, sums) of the kernel, ref = the reference's (cost, dlogits, cost_sum,
    cost_opt)."""
    cost, dl, sums = got
    B = cost.shape[0]
    tag = "%s %s" % (head, " ".join("%s=%s" % (k, v) for k, v in d.items() if not isinstance(v, np.ndarray) and k not in ("q", "weighted")))
    worst = _WORST.setdefault(head, {}).setdefault(d["regime"], {"cost": 0.0, "dlogits": 0.0, "sums": 0.0})
    for name, g, r in (("cost", cost, ref[0]), ("dlogits", dl, ref[1])):
        assert np.all(np.isfinite(g)), (tag, name)
        mag = max(1.0, float(np.abs(r).max()))
        err = float(np.abs(g.astype(np.float64) - r).max())
        worst[name] = max(worst[name], err / mag)
        record_accuracy("%s %s %s" % (head, d["regime"], name), err, C.ARRAY_TOL * mag, mag)
        assert err <= C.ARRAY_TOL * mag, (tag, name, err, C.ARRAY_TOL * mag)
    for k, r in ((0, ref[2]), (1, ref[3])):
        err = abs(float(sums[k]) - r)
        tol = C.SUM_TOL * abs(r) if r != 0.0 else C.SUM_TOL
        if r != 0.0:
            worst["sums"] = max(worst["sums"], err / abs(r))
        record_accuracy("%s %s sums[%d]" % (head, d["regime"], k), err, tol, abs(r))
        assert err <= tol, (tag, "sums[%d]" % k, float(sums[k]), r)
    # reduce_mean over the PADDED batch, formed from the float32 sum by one division
    q = np.float32(sums[0]) / np.float32(B)
    assert abs(np.float32(sums[1]) - q) <= np.spacing(np.abs(q)), (tag, sums, q)
    # masked graphs (and masked tasks) cost nothing and pass no gradient down: exactly 0, not merely small
    mask = d.get("mask")
    if mask is not None:
        dead = mask == 0
        assert np.all(cost[dead] == 0) and np.all(dl[dead] == 0), (tag, "masked rows")
    if zero_elems is not None:
        assert np.all(dl[zero_elems] == 0), (tag, "masked tasks")


@pytest.mark.parametrize("B", C.BATCHES)
def test_sigmoid_head(B):
    """kgcn_masked_sigmoid_ce_f32: T in {1, 5, 12} x {unweighted, scalar 2.5, per-task 0.2 ... 40} x mask_label {NULL, 80 % ones, one
    task off} x graph mask {zero tail, all zero} x logits {N(0, 3), exact grid to +-120, equal rows}."""
    from kgcn_amd._lib import lib, ptr, current_stream
    n = 0
    for d in C.sigmoid_cases(B):
        T = d["T"]
        x, z, mk, ml, qv = _up(d["logits"]), _up(d["labels"]), _up(d["mask"]), _up(d["mask_label"]), _up(d["qvec"])
        got = _run(lambda cost, dl, sums, ws, wsb: lib.kgcn_masked_sigmoid_ce_f32(
            ptr(x), ptr(z), ptr(mk), ptr(ml), B, T, d["weighted"], d["q"], ptr(qv), ptr(cost), ptr(dl), ptr(sums), ptr(ws), wsb,
            current_stream()), B, T)
        ref = R.sigmoid_ce(d["logits"], d["labels"], d["mask"], d["mask_label"], d["pos_weight"])
        _check("sigmoid", d, got, ref, None if d["mask_label"] is None else d["mask_label"] == 0)
        n += 1
    assert n == 3 * 3 * 3 * 2 * 3
    print("sigmoid head B=%d: largest errors so far %s" % (B, _WORST["sigmoid"]))


@pytest.mark.parametrize("B", C.BATCHES)
def test_softmax_head(B):
    """kgcn_masked_softmax_ce_f32: C in {1, 2, 5, 33} x labels {one-hot, soft rows summing to 1, to 0.3 and 2, all-zero rows} x graph
    mask {zero tail, all zero} x logits {N(0, 3), exact grid, equal rows, rows with a spread of 200}."""
    from kgcn_amd._lib import lib, ptr, current_stream
    n = 0
    for d in C.softmax_cases(B):
        W = d["C"]
        x, z, mk = _up(d["logits"]), _up(d["labels"]), _up(d["mask"])
        got = _run(lambda cost, dl, sums, ws, wsb: lib.kgcn_masked_softmax_ce_f32(
            ptr(x), ptr(z), ptr(mk), B, W, ptr(cost), ptr(dl), ptr(sums), ptr(ws), wsb, current_stream()), B, W)
        _check("softmax", d, got, R.softmax_ce(d["logits"], d["labels"], d["mask"]))
        if d["label_kind"] == "zero_rows":            # a row without any label: no cost and, with sum_c z = 0, no gradient
            assert np.all(got[0][::3] == 0) and np.all(got[1][::3] == 0)
        n += 1
    assert n == 4 * 4 * 2 * 4 - 4 * 2
    print("softmax head B=%d: largest errors so far %s" % (B, _WORST["softmax"]))


@pytest.mark.parametrize("B", C.BATCHES)
def test_sparse_softmax_head(B):
    """kgcn_sparse_softmax_ce_f32: the same C and logits, class indices that include 0 and C - 1, mask NULL / zero tail / all zero
    (ops.py always passes NULL)."""
    from kgcn_amd._lib import lib, ptr, current_stream
    n = 0
    for d in C.sparse_cases(B):
        W = d["C"]
        assert d["idx"][-1] == W - 1 and (B == 1 or d["idx"][0] == 0)          # one row has room for one of the two
        x, idx, mk = _up(d["logits"]), _up(d["idx"]), _up(d["mask"])
        got = _run(lambda cost, dl, sums, ws, wsb: lib.kgcn_sparse_softmax_ce_f32(
            ptr(x), ptr(idx), ptr(mk), B, W, ptr(cost), ptr(dl), ptr(sums), ptr(ws), wsb, current_stream()), B, W)
        _check("sparse", d, got, R.sparse_softmax_ce(d["logits"], d["idx"], d["mask"]))
        n += 1
    assert n == 4 * 3 * 4 - 3
    print("sparse head B=%d: largest errors so far %s" % (B, _WORST["sparse"]))


def test_heads_refuse_bad_arguments_before_launching():
    from kgcn_amd._lib import lib, ptr, current_stream
    t = torch.zeros(64, device=dev())
    i = torch.zeros(8, dtype=torch.int64, device=dev())
    s = current_stream()
    assert lib.kgcn_masked_sigmoid_ce_f32(ptr(t), ptr(t), ptr(t), None, 0, 4, 0, 0.0, None, None, ptr(t), ptr(t), ptr(t), 256, s) != 0
    assert lib.kgcn_masked_sigmoid_ce_f32(ptr(t), ptr(t), None, None, 8, 4, 0, 0.0, None, None, ptr(t), ptr(t), ptr(t), 256, s) != 0
    assert lib.kgcn_masked_softmax_ce_f32(ptr(t), ptr(t), ptr(t), 300, 2, None, ptr(t), ptr(t), ptr(t), 4, s) != 0     # two partials
    assert b"workspace" in lib.kgcn_last_error()
    assert lib.kgcn_sparse_softmax_ce_f32(ptr(t), None, None, 8, 4, None, ptr(t), ptr(t), ptr(t), 256, s) != 0
    assert lib.kgcn_sparse_softmax_ce_f32(ptr(t), ptr(i), None, 8, 0, None, ptr(t), ptr(t), ptr(t), 256, s) != 0
    torch.cuda.synchronize()
    assert bool((t == 0).all())


# ---- loss_grad_kernel through autograd: cost_opt alone, cost_sum alone (g_opt is None), both ------------------------------------
def _autograd(loss_of, logits, upstream):
    a, b = upstream
    x = _up(logits).requires_grad_(True)
    cost_opt, cost_sum = loss_of(x)
    if (a, b) == (1.0, 0.0):
        cost_opt.backward()
    elif (a, b) == (0.0, 1.0):
        cost_sum.backward()                       # cost_opt takes no part: its upstream gradient really is None
    else:
        (a * cost_opt + b * cost_sum).backward()
    return x.grad.cpu().numpy(), float(cost_opt.detach()), float(cost_sum.detach())


def _check_grad(what, got, ref):
    mag = max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(got.astype(np.float64) - ref).max())
    record_accuracy(what, err, C.ARRAY_TOL * mag, mag)
    assert err <= C.ARRAY_TOL * mag, (what, err, C.ARRAY_TOL * mag)


@pytest.mark.parametrize("upstream", C.AUTOGRAD_UPSTREAM, ids=["opt", "sum", "both"])
@pytest.mark.parametrize("regime", ["normal", "grid"])
def test_autograd_masked_sigmoid_ce(regime, upstream):
    from kgcn_amd import ops
    d = C.autograd_sigmoid_case(regime)
    z, mk, ml = _up(d["labels"]), _up(d["mask"]), _up(d["mask_label"])
    got, co, cs = _autograd(lambda x: ops.masked_sigmoid_ce(x, z, mk, ml, d["qvec"]), d["logits"], upstream)
    ref = R.sigmoid_ce(d["logits"], d["labels"], d["mask"], d["mask_label"], d["qvec"])
    a, b = upstream
    _check_grad("sigmoid autograd %s" % regime, got, R.loss_grad(ref[1], a if a else None, b if b else None, d["B"]))
    assert abs(cs - ref[2]) <= C.SUM_TOL * ref[2] and abs(co - ref[3]) <= C.SUM_TOL * ref[3]
    assert np.all(got[d["mask"] == 0] == 0)


@pytest.mark.parametrize("upstream", C.AUTOGRAD_UPSTREAM, ids=["opt", "sum", "both"])
@pytest.mark.parametrize("regime", ["normal", "grid"])
def test_autograd_masked_softmax_ce(regime, upstream):
    from kgcn_amd import ops
    d = C.autograd_softmax_case(regime)
    z, mk = _up(d["labels"]), _up(d["mask"])
    got, co, cs = _autograd(lambda x: ops.masked_softmax_ce(x, z, mk), d["logits"], upstream)
    ref = R.softmax_ce(d["logits"], d["labels"], d["mask"])
    a, b = upstream
    _check_grad("softmax autograd %s" % regime, got, R.loss_grad(ref[1], a if a else None, b if b else None, d["B"]))
    assert abs(cs - ref[2]) <= C.SUM_TOL * ref[2] and abs(co - ref[3]) <= C.SUM_TOL * ref[3]


@pytest.mark.parametrize("regime", ["normal", "grid"])
def test_autograd_sparse_softmax_ce_sum_with_an_upstream_factor(regime):
    from kgcn_amd import ops
    d = C.autograd_sparse_case(regime)
    x = _up(d["logits"]).requires_grad_(True)
    s = ops.sparse_softmax_ce_sum(x, _up(d["idx"]))
    (3.0 * s).backward()
    ref = R.sparse_softmax_ce(d["logits"], d["idx"])
    _check_grad("sparse autograd %s" % regime, x.grad.cpu().numpy(), R.loss_grad(ref[1], None, 3.0, 1))
    assert abs(float(s.detach()) - ref[2]) <= C.SUM_TOL * ref[2]
