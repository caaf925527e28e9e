"""tests/seqcnn_ig_oracle.py on the CPU: the completeness of the oracle's integrated gradients, the linearity identities the fused
route of kgcn_amd.visualization.seqcnn_integrated_gradients rests on, the refusals of the public functions before any device
use, and the new names of the C ABI."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import seqcnn_ig_oracle as IO  # noqa: E402
import seqcnn_oracle as O  # noqa: E402

S, E, L = 26, 25, 50
NARROW = (33, 20, 12)


def _protein(seed=3):
    p, tokens, _ = IO.draw_case(seed, S, E, L, 1, NARROW)
    return p, np.asarray(p["embeddings"], np.float64)[tokens[0]]


def test_completeness_excess_falls_with_the_step_count():
    p, e = _protein()
    mask = np.array([0.0, 1.0])
    excess = []
    for D in (8, 64, 512):
        r = IO.integrated_gradients(p, e, mask, "ig", D)
        excess.append(abs(r["sum"] - (r["end"] - r["start"])))
    print("SEQCNN_IG completeness excess at D = 8, 64, 512:", excess, "end - start", r["end"] - r["start"])
    assert excess[0] > excess[1] > excess[2]
    assert excess[2] < 1e-2 * abs(r["end"] - r["start"])


def test_score_gradient_agrees_with_central_differences():
    p, e = _protein(5)
    mask = np.array([[0.3, 1.0]])
    x = (0.7 * e)[None]
    _, g, _ = IO.score_grad(p, x, mask)
    rng = np.random.default_rng(1)
    d = rng.standard_normal(x.shape)
    h = 1e-6
    sp, sm = IO.score_grad(p, x + h * d, mask, False)[0], IO.score_grad(p, x - h * d, mask, False)[0]
    num, ana = float((sp - sm)[0]) / (2 * h), float((g * d).sum())
    assert abs(num - ana) <= 1e-6 * max(abs(num), abs(ana), 1e-3), (num, ana)


def test_linearity_identities_of_the_fused_route():
    """In fp64: conv(alpha e) + b = alpha P + b with P = conv(e) without bias; the window maximum commutes with p -> relu(alpha p +
    b) for alpha >= 0; and sum_k w_k conv^T(dpre_k) = conv^T(sum_k w_k dpre_k), with the gradient routed to the arg-max of P."""
    rng = np.random.default_rng(11)
    B, Lc, Cin, F, k, pool = 2, 22, 7, 9, 4, 4
    e = rng.standard_normal((B, Lc, Cin))
    w, b = rng.standard_normal((k, Cin, F)) / 3, rng.uniform(-0.3, 0.3, F)
    zero = np.zeros(F)
    cP = O.conv1d_pool_fwd(w, zero, pool, None, x=e)
    alphas, weights = [0.0, 0.25, 0.5, 1.0, 1.75], [0.0, 0.3, 0.2, 0.4, 0.1]
    T = Lc // pool
    acc_dx, r = np.zeros_like(e), np.zeros((B, T, F))
    for a, wk in zip(alphas, weights):
        ck = O.conv1d_pool_fwd(w, b, pool, "relu", x=a * e)
        assert np.abs(ck["pre"] - (a * cP["pre"] + b)).max() <= 1e-12
        fused_out = np.maximum(a * cP["out"] + b, 0.0)
        assert np.abs(ck["out"] - fused_out).max() <= 1e-12
        dout = rng.standard_normal((B, T, F))
        if wk != 0.0:
            live = ck["out"] > 0
            if a > 0:                   # where the unit is live and the scale positive, the composed arg-max is P's
                assert np.array_equal(ck["arg"][live], cP["arg"][live])
            acc_dx += wk * O.conv1d_pool_bwd(ck, dout)["dx"]
            r += wk * dout * (fused_out > 0)
    fused_dx = O.conv1d_pool_bwd(cP, r)["dx"]
    assert np.abs(fused_dx - acc_dx).max() <= 1e-12 * max(1.0, np.abs(acc_dx).max())


def test_fp32_sweeps_restate_the_header():
    rng = np.random.default_rng(2)
    Pm = rng.standard_normal((2, 3, 5)).astype(np.float32)
    bias = rng.uniform(-0.5, 0.5, 5).astype(np.float32)
    alpha = np.array([0.0, 0.5, 1.0], np.float32)
    out = IO.expand32(Pm, alpha, bias)
    assert out.shape == (6, 3, 5) and out.dtype == np.float32
    assert np.array_equal(out[2], np.maximum(Pm[0] + bias, 0))                       # alpha 1: the layer's own bias add
    assert np.array_equal(out[0], np.broadcast_to(np.maximum(bias, 0), (3, 5)))
    assert not np.signbit(out).any()
    dout = rng.standard_normal(out.shape).astype(np.float32)
    w = np.array([0.0, 0.25, 0.5], np.float32)
    dout[0::3] = np.nan                                                              # the weight-0 copies are never read
    r = IO.reduce32(dout, out, w)
    ref = np.zeros((2, 3, 5), np.float32)
    for c in range(2):
        for k in (1, 2):
            ref[c] = np.where(out[c * 3 + k] > 0, ref[c] + w[k] * dout[c * 3 + k], ref[c])
    assert np.array_equal(r, ref) and np.isfinite(r).all()


def test_public_functions_refuse_on_the_host():
    import torch
    import kgcn  # noqa: F401  (the alias package resolves to the same modules)
    from kgcn_amd import models, ops, visualization as V
    tokens = torch.zeros((2, L), dtype=torch.int32)
    with pytest.raises(TypeError, match="GCN"):
        V.seqcnn_integrated_gradients(models.GCN(1, 2), tokens)
    model = models.SeqCNN(S, embedding_dim=E)
    for method in V.SMOOTH_METHODS:
        with pytest.raises(ValueError, match="fused"):
            V.seqcnn_integrated_gradients(model, tokens, method=method, fused=True)
    with pytest.raises(ValueError):
        V.seqcnn_integrated_gradients(model, tokens, method="deeplift")
    with pytest.raises(ValueError):
        V.seqcnn_integrated_gradients(model, tokens, divide_number=0)
    with pytest.raises(ValueError):
        V.seqcnn_integrated_gradients(model, tokens, chunk=0)
    Pm, bias = torch.zeros((1, 2, 3)), torch.zeros(3)
    for bad in ([0.5, -0.25], [float("nan")], [float("inf")], [], [0.0] * (ops.CONV1D_IG_MAX_COPIES + 1)):
        with pytest.raises(ValueError):
            ops.conv1d_ig_expand(Pm, bad, bias)
    with pytest.raises(ValueError):
        ops.conv1d_ig_reduce(Pm, Pm, [])
    assert ops.CONV1D_IG_MAX_COPIES == 1024
    assert isinstance(V.SEQCNN_IG_FUSED, bool)


def test_abi_names_are_in_the_header():
    from kgcn_amd import _lib
    text = open(os.path.join(ROOT, "include", "kgcn_hip.h")).read()
    for name in ("kgcn_ig_conv1d_expand_f32", "kgcn_ig_conv1d_reduce_f32"):
        assert name in _lib.SIGNATURES and name in text
        assert hasattr(_lib.lib, name)
    assert _lib.K["KGCN_CONV1D_IG_MAX_COPIES"] == 1024
    assert len(_lib.SIGNATURES["kgcn_ig_conv1d_expand_f32"][1]) == 9 and len(_lib.SIGNATURES["kgcn_ig_conv1d_reduce_f32"][1]) == 9
    assert "entry points only, version still 2" in text[text.index("kgcn_ig_conv1d_expand_f32"):]
