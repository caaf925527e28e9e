"""The cross-layer stack kernels (csrc/stack.hip: one graph per workgroup trip; csrc/stack_tile.hip: 64-row tiles on the f32
MFMA) against the fp64 reference of a layer list (tests/stack_oracle.py), called through ops.gcn_stack on every route, on the
lists of tests/stack_cases.py: all four activations and their derivatives, normalisations first / twice, changing widths,
contraction widths 1..3 and 64, NULL biases, no dx, per-node output, one-node and dense 32-node graphs, duplicates, second
trips.  models.GCN (tests/test_gpu_model.py) reaches the same kernels with one list only.
"""
import numpy as np
import pytest
import torch

import stack_cases as C
import stack_oracle as S
from test_gpu_parity import close, dev, t32

pytestmark = pytest.mark.gpu

# No comparison is looser than atol + rel * max|ref| (the loosest relative tolerance the stack tests of test_gpu_model.py apply
# to the same quantities) ...
ATOL, REL = 1e-6, 2e-5
# ... and each is held to TEN TIMES the error it measured, never below conftest.FP32_FLOOR (the tolerance ratchet).
# Measured on the MI355X, largest |error| / max(1, max|ref|) per (case, kernels) and tensor kind, rounded down
# (profiles/layer_lists_stack_accuracy.json); routes 0 and 2 run the same (tile) kernels and measured the same, bit for bit.
MEASURED = {
    ("relu_chain", "one_graph"): {"forward": 8.30e-08, "dx": 1.68e-07, "dW": 2.17e-07, "db": 1.31e-07},
    ("relu_chain", "tile"): {"forward": 1.41e-07, "dx": 1.01e-07, "dW": 1.72e-07, "db": 1.30e-07},
    ("tanh_identity_per_node", "one_graph"): {"forward": 4.31e-07, "dx": 1.81e-07, "dW": 3.10e-07, "db": 2.00e-07, "dgamma": 8.42e-08, "dbeta": 2.14e-07},
    ("tanh_identity_per_node", "tile"): {"forward": 2.87e-07, "dx": 1.45e-07, "dW": 3.10e-07, "db": 2.13e-07, "dgamma": 8.69e-08, "dbeta": 1.63e-07},
    ("norm_first_offset", "one_graph"): {"forward": 6.98e-08, "dx": 1.46e-07, "dW": 2.19e-07, "db": 2.79e-07, "dgamma": 2.19e-07, "dbeta": 1.57e-07},
    ("norm_first_offset", "tile"): {"forward": 3.15e-07, "dx": 1.37e-07, "dW": 3.86e-07, "db": 1.16e-07, "dgamma": 1.79e-07, "dbeta": 9.51e-08},
    ("two_norms_ragged_tile", "one_graph"): {"forward": 1.40e-07, "dx": 9.76e-08, "dW": 2.96e-07, "db": 3.23e-07, "dgamma": 1.33e-07, "dbeta": 3.42e-07},
    ("two_norms_ragged_tile", "tile"): {"forward": 1.36e-07, "dx": 8.27e-08, "dW": 3.91e-07, "db": 3.07e-07, "dgamma": 2.08e-07, "dbeta": 2.25e-07},
    ("eight_layers", "one_graph"): {"forward": 1.05e-07, "dx": 1.99e-08, "dW": 3.87e-07, "db": 3.14e-07, "dgamma": 1.93e-07, "dbeta": 2.30e-07},
    ("one_node", "one_graph"): {"forward": 7.09e-08, "dx": 1.15e-07, "dW": 1.38e-07, "db": 1.13e-07},
    ("one_node", "tile"): {"forward": 8.57e-08, "dx": 7.71e-08, "dW": 1.74e-07, "db": 1.37e-07},
    ("narrow", "one_graph"): {"forward": 5.55e-08, "dx": 1.19e-07, "dW": 1.44e-07, "db": 3.88e-07},
    ("narrow", "tile"): {"forward": 9.05e-08, "dx": 8.73e-08, "dW": 2.82e-07, "db": 1.87e-07},
    ("no_bias_no_dx", "one_graph"): {"forward": 7.23e-08, "dW": 2.12e-07},
    ("no_bias_no_dx", "tile"): {"forward": 1.50e-07, "dW": 1.60e-07},
    ("dense32", "one_graph"): {"forward": 2.22e-08, "dx": 7.17e-09, "dW": 6.18e-08, "db": 2.33e-07},
    ("dense32", "tile"): {"forward": 5.93e-08, "dx": 7.17e-09, "dW": 5.21e-08, "db": 1.79e-07},
    ("dense32_duplicate", "one_graph"): {"forward": 4.65e-08, "dx": 5.76e-09, "dW": 5.11e-08, "db": 1.27e-07},
    ("dense32_duplicate", "tile"): {"forward": 5.18e-08, "dx": 5.76e-09, "dW": 4.18e-08, "db": 1.27e-07},
    ("second_trips_tiles", "one_graph"): {"forward": 1.70e-07, "dx": 1.57e-07, "dW": 1.85e-07, "db": 2.04e-07},
    ("second_trips_tiles", "tile"): {"forward": 2.91e-07, "dx": 1.57e-07, "dW": 1.66e-07, "db": 1.35e-07},
    ("second_trips_one_graph", "one_graph"): {"forward": 1.07e-07, "dx": 1.32e-07, "dW": 1.36e-07, "db": 2.51e-07},
    ("second_trips_one_graph", "tile"): {"forward": 1.21e-07, "dx": 1.04e-07, "dW": 1.53e-07, "db": 1.14e-07},
    ("module_list", "tile"): {"forward": 1.35e-07, "dx": 1.45e-07, "parameter gradients": 1.88e-07},
}


def _close(got, ref, key, kind, what):
    """close() at min(the written tolerance, 10 x the measured error of this comparison, floored at FP32_FLOOR)"""
    import conftest
    mag = float(np.abs(ref).max())
    tol = max(10.0 * MEASURED[key][kind], conftest.FP32_FLOOR) * max(1.0, mag)
    return close(got, ref, atol=min(ATOL + REL * mag, tol), what="%s: %s" % (what, kind))


def _tensors(case):
    """the case on the device -> (d, csr, x, params, buffers, enabled)"""
    from kgcn_amd.batched_csr import BatchedCSR
    d = C.make_case(case)
    N = d["x"].shape[1]
    csr = BatchedCSR.from_coo_list([a[0] for a in d["adjs"]], rows=N, cols=N, device=dev())
    x = t32(d["x"])
    if d["dx"]:
        x.requires_grad_(True)
    params = [None if p is None else t32(p).requires_grad_(True) for p in d["params"]]
    buffers = tuple(None if b is None else (t32(b[0]), t32(b[1])) for b in d["buffers"])
    has_norm = any(s[0] == S.NORM for s in d["spec"])
    enabled = torch.as_tensor(d["sizes"], dtype=torch.int32, device=dev()) if has_norm and d["sizes"] is not None else None
    return d, csr, x, params, buffers, enabled


def _run(case, route, repeats=1):
    """forward and backward on `route`, `repeats` times -> (d, out, d x, [parameter gradients] of every run), or None when the
    route does not take the list (kgcn_gcn_stack_supported must say what the table says)"""
    from kgcn_amd import ops
    d, csr, x, params, buffers, enabled = _tensors(case)
    ops.stack_route = route
    try:
        supported = ops.gcn_stack_supported(csr, d["spec"])
        assert supported == (route in d["routes"]), (case, route, supported)
        if not supported:
            return None
        runs = []
        for _ in range(repeats):
            for t in [p for p in params if p is not None] + [x]:
                t.grad = None
            out = ops.gcn_stack(x, csr, enabled, d["spec"], buffers, d["gather"], params)
            assert "GcnStack" in out.grad_fn.__class__.__name__, out.grad_fn
            out.backward(t32(d["cotangent"]))
            runs.append([None if p is None else p.grad.clone() for p in params])
        return d, out.detach(), x.grad, runs
    finally:
        ops.stack_route = 0


def _dgamma_bound(d, l):
    """Worst-case error of an fp32 running sum of the terms of dgamma = rstd (sum dpre x - mean sum dpre), per column:
    (n + 2) 2^-24 rstd (sum |dpre x| + |mean| sum |dpre|), the sums from the fp64 reference over the n valid rows."""
    kind, act, din, dout, eps = d["spec"][l]
    assert l == 0 and kind == S.NORM
    hin = np.asarray(d["x"], np.float64)
    mean, var = (np.asarray(b, np.float64) for b in d["buffers"][0])
    rstd = 1.0 / np.sqrt(var + eps)
    # the layer's d pre-activation from the reference's dx = gamma rstd dpre (0 on the padded rows)
    dpre = d["ref"]["dx"] / (np.asarray(d["params"][0], np.float64) * rstd)
    n = int(d["sizes"].sum())
    return (n + 2) * 2.0 ** -24 * rstd * (np.abs(dpre * hin).sum((0, 1)) + np.abs(mean) * np.abs(dpre).sum((0, 1)))


@pytest.mark.parametrize("route", [0, 1, 2])
@pytest.mark.parametrize("case", list(C.CASES))
def test_stack_against_fp64_reference(case, route):
    """Forward output, dx and every parameter gradient for a random-normal cotangent.  A route that does not take the list
    (the tile route keeps dW accumulators for four matrices: the eight-layer list has five) must say so in
    kgcn_gcn_stack_supported and refuse the call; route 0 then runs the one-graph kernels.  The first two cases run the
    backward twice: fixed-order reductions, bit-identical parameter gradients."""
    from kgcn_amd import _lib, ops
    repeats = 2 if case in ("relu_chain", "tanh_identity_per_node") else 1
    res = _run(case, route, repeats)
    if res is None:
        d, csr, x, params, buffers, enabled = _tensors(case)
        ops.stack_route = route
        try:
            with pytest.raises(_lib.KgcnHipError):           # refused on the host, before any launch
                ops.gcn_stack(x, csr, enabled, d["spec"], buffers, d["gather"], params)
        finally:
            ops.stack_route = 0
        return
    d, out, dx, runs = res
    ref = d["ref"]
    key = (case, "one_graph" if route == 1 or 2 not in d["routes"] else "tile")
    _close(out, ref["out"], key, "forward", "stack")
    if d["dx"]:
        _close(dx, ref["dx"], key, "dx", "stack")
    else:
        assert dx is None
    names = {S.CONV: ("dW", "db"), S.DENSE: ("dW", "db"), S.NORM: ("dgamma", "dbeta")}
    for i, g in enumerate(runs[0]):
        l, kind = i // 2, d["spec"][i // 2][0]
        if d["params"][i] is None:
            assert g is None                                 # a NULL bias has no gradient
            continue
        assert tuple(g.shape) == d["params"][i].shape
        _close(g, ref["grads"][i], key, names[kind][i % 2], "stack")
        if case == "norm_first_offset" and l == 0 and i % 2 == 0:
            err = np.abs(g.cpu().numpy().astype(np.float64) - ref["grads"][i])
            bound = _dgamma_bound(d, 0)
            print("dgamma, offset data: max err / derived bound per column %.3g (err %.3g, bound %.3g)"
                  % ((err / bound).max(), err.max(), bound.min()))
            assert (err <= bound).all(), (err, bound)        # measured: at most 6.5e-4 of the bound (err 6.5e-7), both kernels
    for again in runs[1:]:
        for a, b in zip(runs[0], again):
            assert (a is None and b is None) or torch.equal(a, b)


def test_route_selection_is_bitwise_visible():
    """Route 0 runs the tile kernels whenever they take the list and the one-graph kernels otherwise: its results are
    bit-identical to the forced route of the same kernels (both are deterministic)."""
    for case, same in (("eight_layers", 1), ("relu_chain", 2)):
        auto, forced = _run(case, 0), _run(case, same)
        assert torch.equal(auto[1], forced[1]) and torch.equal(auto[2], forced[2]), case
        for a, b in zip(auto[3][0], forced[3][0]):
            assert torch.equal(a, b), case


def test_fused_stack_module_list_against_reference():
    """layers.fused_stack, the public entry, on [GraphConv(relu), GraphBatchNormalization(tanh), GraphDense(None)] built
    Keras-style: a module list other than models.GCN's, true sizes, per-node output."""
    from kgcn_amd import layers
    d = C.make_case("module_list")
    ref, (_, _, d0, w1, _), w2 = d["ref"], d["spec"][0], d["spec"][2][3]
    seq = [layers.GraphConv(w1, 1, activation="relu"), layers.GraphBatchNormalization(activation="tanh", eps=C.EPS),
           layers.GraphDense(w2, activation=None)]
    for m, din in zip(seq, (d0, w1, w1)):
        m.build((None, None, din), dev())
    ps = [seq[0].w[0], seq[0].bias[0], seq[1].gamma, seq[1].beta, seq[2].kernel, seq[2].bias]
    with torch.no_grad():
        for p, v in zip(ps, d["params"]):
            assert tuple(p.shape) == v.shape
            p.copy_(t32(v))
        seq[1].moving_mean.copy_(t32(d["buffers"][1][0]))
        seq[1].moving_variance.copy_(t32(d["buffers"][1][1]))
    x = t32(d["x"]).requires_grad_(True)
    out = layers.fused_stack(seq, x, d["adjs"], enabled_node_nums=torch.as_tensor(d["sizes"]), gather=False)
    assert out is not None and "GcnStack" in out.grad_fn.__class__.__name__
    out.backward(t32(d["cotangent"]))
    key = ("module_list", "tile")
    _close(out, ref["out"], key, "forward", "fused_stack")
    _close(x.grad, ref["dx"], key, "dx", "fused_stack")
    for p, g in zip(ps, ref["grads"]):
        _close(p.grad, g, key, "parameter gradients", "fused_stack")


def test_fused_stack_returns_none_for_ineligible_inputs():
    from kgcn_amd import layers
    rng = np.random.default_rng(7)

    def batch(T, N, d0, channels=1):
        adjs = [[(np.array([[0, 1], [1, 0]], np.int64), np.array([0.5, -0.5], np.float32), [N, N])] * channels for _ in range(T)]
        return t32(rng.standard_normal((T, N, d0))), adjs

    def built(mods, x, adjs):
        d = x.shape[2]                                       # Keras-style: parameters exist once the layer is built
        for m in mods:
            m.build((None, None, d), dev())
            d = getattr(m, "output_dim", d)
        return mods

    x, adjs = batch(4, 8, 6)
    ok = built([layers.GraphConv(9, 1, activation="relu"), layers.GraphDense(5)], x, adjs)
    assert layers.fused_stack(ok, x, adjs, gather=False) is not None            # the control: this list IS eligible
    x33, adjs33 = batch(4, 33, 6)
    assert layers.fused_stack(built([layers.GraphConv(9, 1), layers.GraphDense(5)], x33, adjs33), x33, adjs33) is None     # N = 33
    assert layers.fused_stack(built([layers.GraphConv(65, 1), layers.GraphDense(5)], x, adjs), x, adjs) is None            # width 65
    nine = built([layers.GraphConv(9, 1)] + [layers.GraphDense(9) for _ in range(8)], x, adjs)
    assert layers.fused_stack(nine, x, adjs) is None and layers.fused_stack(nine[:8], x, adjs) is not None                 # nine layers
    bn = built([layers.GraphConv(9, 1), layers.GraphBatchNormalization(learning_phase=0), layers.GraphDense(5)], x, adjs)
    assert layers.fused_stack(bn, x, adjs) is not None
    bn[1].learning_phase = 1
    assert layers.fused_stack(bn, x, adjs) is None                                                                         # learning phase 1
    x2, adjs2 = batch(4, 8, 6, channels=2)
    assert layers.fused_stack(built([layers.GraphConv(9, 2), layers.GraphDense(5)], x2, adjs2), x2, adjs2) is None         # two channels
