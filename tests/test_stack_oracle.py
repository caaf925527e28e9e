"""CPU checks of tests/stack_oracle.py, the fp64 reference the cross-layer stack kernels are compared with
(tests/test_gpu_stack_layers.py): its gradients against central differences, and the relu margin of every GPU case."""
import numpy as np
import pytest

import stack_cases as C
import stack_oracle as S


def _loss(d, params, x):
    return float((S.stack_forward(d["spec"], params, d["buffers"], x, d["adjs"], d["sizes"], d["gather"])[2] * d["cotangent"]).sum())


@pytest.mark.parametrize("case", sorted(C.SMALL))
def test_reference_gradients_by_central_differences(case):
    """d <out, cotangent> / d (x, every parameter) of the reference against (L(v + h) - L(v - h)) / 2h in fp64, h = 1e-5: the
    truncation error is h^2 f''' / 6 ~ 1e-10 and the rounding error eps |L| / h ~ 1e-10 for values of order 1, so 1e-7 of
    max(1, |gradient|) is a thousand times both.  fd_smooth: tanh conv, sigmoid normalisation with true sizes, identity
    dense, read-out; fd_relu: relu on all three kinds, per-node output -- every nonzero relu pre-activation is at least 1e-3
    away from the kink, a hundred steps."""
    d = C.make_case(case)
    h = 1e-5
    for l, (kind, act, din, dout, eps) in enumerate(d["spec"]):
        if act == S.ACT_RELU:
            z = np.abs(d["ref"]["pre"][l])
            assert z[z != 0].min() >= 1e-3, (case, l, z[z != 0].min())
    params = [np.array(p, np.float64) for p in d["params"]]
    x = np.array(d["x"], np.float64)
    ref = d["ref"]

    def numeric(arr):
        g = np.zeros_like(arr)
        flat, gf = arr.reshape(-1), g.reshape(-1)
        for i in range(flat.size):
            keep = flat[i]
            flat[i] = keep + h
            up = _loss(d, params, x)
            flat[i] = keep - h
            gf[i] = (up - _loss(d, params, x)) / (2 * h)
            flat[i] = keep
        return g

    for what, arr, got in [("dx", x, ref["dx"])] + [("param %d" % i, p, ref["grads"][i]) for i, p in enumerate(params)]:
        num = numeric(arr)
        assert np.abs(num - got).max() <= 1e-7 * max(1.0, np.abs(num).max()), (case, what, np.abs(num - got).max())
    # the flat layout of the ABI: dW | db per matrix layer, dgamma | dbeta per normalisation
    assert np.array_equal(ref["dparams"], np.concatenate([g.ravel() for g in ref["grads"]]))
    # a normalisation's padded rows pass nothing down; the read-out reaches every row
    if case == "fd_relu":
        pad = np.arange(x.shape[1])[None, :] >= d["graph_sizes"][:, None]
        assert pad.any() and (ref["outs"][1][pad] == 0).all()          # relu(0)


def test_padded_rows_behind_a_normalisation_are_act_of_zero():
    d = C.make_case("fd_smooth")
    pad = np.arange(d["x"].shape[1])[None, :] >= d["graph_sizes"][:, None]
    assert pad.any() and (d["ref"]["outs"][1][pad] == 0.5).all()       # sigmoid(0)
    assert np.array_equal(d["ref"]["out"], d["ref"]["outs"][-1].sum(1))  # the read-out sums ALL rows


@pytest.mark.parametrize("case", sorted(C.CASES) + sorted(C.MODULES))
def test_relu_margin(case):
    """A relu whose pre-activation the fp32 kernels round to the other side of 0 flips its mask: a mismatch that says nothing
    about the kernels.  The fp32 evaluation differs from fp64 by 1e-7 .. 5e-7 of the tensor's maximum, so every pre-activation
    of a relu layer must be exactly 0 (rows without entries, padded rows) or at least 1e-5 in magnitude -- twenty times that.  A
    seed that does not meet this fails HERE, never as a GPU mismatch."""
    assert C.relu_margin_violations(case) == [], case


@pytest.mark.parametrize("case", sorted(C.CASES))
def test_case_inputs(case):
    """what the table promises: an empty and a full-size graph, zero feature rows behind the sizes, and the stated extremes"""
    d, c = C.make_case(case), C.CASES[case]
    n = d["graph_sizes"]
    N = c["N"]
    assert (n == N).any() and (c.get("graphs", "").startswith("dense") or (n == 0).any())
    assert not d["x"][np.arange(N)[None, :] >= n[:, None]].any()
    per_row = max(np.bincount(a[0][0][:, 0], minlength=N).max() if len(a[0][0]) else 0 for a in d["adjs"])
    if c.get("graphs") == "dense":
        assert per_row == N and all(len(a[0][1]) == N * N for a in d["adjs"])
    if c.get("graphs") == "dense_dup":
        assert per_row == N + 1 and sorted(len(a[0][1]) for a in d["adjs"])[-2:] == [N * N, N * N + 1]
    if c.get("data") == "offset":
        assert abs(d["x"][d["x"] != 0].mean() - 4.0) < 0.2 and abs(d["buffers"][0][0].mean() - 4.0) < 0.2
