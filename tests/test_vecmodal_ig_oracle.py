"""tests/vecmodal_ig_oracle.py against itself (no GPU): the closed form of the fused route equals the literal loop of
kgcn/visualization.py:187-260, the hand-written input gradients agree with central differences, the regression model has no
adjacency gradient, the parameter seeds of the GPU tests keep every relu unit off zero -- and the host-side refusals of
visualization.vecmodal_integrated_gradients, which need the library but no device."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vecmodal_ig_oracle as IO  # noqa: E402

Z = np.load(os.path.join(ROOT, "tests", "golden", "g12_vecmodal.npz"), allow_pickle=False)
KINDS = ("vec", "regression")


def _compound(kind, g):
    P, X, A, V, sizes = IO.case(kind, Z)
    return P, X[g], A[g], V[g], None if sizes is None else int(sizes[g])


def _modals(kind):
    return IO.modal_targets(kind, "all")[0] + ("all",)


def _noise(method, g, x, A, v):
    return IO.host_noise(IO.NOISE_SEED, g, IO.DIVIDE, x.shape, A, v.shape[0]) if method in IO.SMOOTH else None


@pytest.mark.parametrize("kind", KINDS)
def test_closed_form_equals_the_literal_loop(kind):
    worst = 0.0
    for g in IO.COMPOUNDS[:3]:
        P, x, A, v, size = _compound(kind, g)
        for mask in (np.array([1.0, 0.0]), np.array([0.0, 1.0])):
            for modal in _modals(kind):
                for method in IO.METHODS:
                    nz = _noise(method, g, x, A, v)
                    a = IO.literal(kind, P, x, A, v, mask, modal, method, IO.DIVIDE, size, nz, IO.NOISE_SCALE)
                    b = IO.closed_form(kind, P, x, A, v, mask, modal, method, IO.DIVIDE, size, nz, IO.NOISE_SCALE)
                    assert sorted(a) == sorted(b)
                    for key in a:
                        if key.endswith("_IG") or key in ("start", "end", "sum_of_IG"):
                            big = np.abs(np.asarray(a[key])).max()
                            err = np.abs(np.asarray(a[key]) - np.asarray(b[key])).max() / (big if big > 0 else 1.0)
                            worst = max(worst, err)
                            assert err <= 1e-12, (kind, g, modal, method, key, err)
                    name = IO.modal_targets(kind, modal)[1]
                    if name + "_IG" in a:
                        assert a[name + "_IG"].shape == (1, v.shape[0]) and a[name].shape == (v.shape[0],)
    print("closed form vs literal loop, %s: worst relative difference %.2e" % (kind, worst))


@pytest.mark.parametrize("kind", KINDS)
def test_input_gradients_agree_with_central_differences(kind):
    rng = np.random.default_rng(5)
    for g in (0, 1):
        P, x, A, v, size = _compound(kind, g)
        mask = np.array([0.3, 1.0])
        x, v = x.astype(np.float64), v.astype(np.float64)
        _, grads = IO.score_grads(kind, P, x, A, v, mask, size)
        f = lambda x_, A_, v_: IO.score_grads(kind, P, x_, A_, v_, mask, size)[0]
        h = 1e-6
        for name, base in (("features", x), ("adjs", A), ("vector", v)):
            picks = np.argwhere(A != 0) if name == "adjs" else np.argwhere(np.ones_like(base))
            picks = picks[rng.permutation(len(picks))[:12]]
            for idx in map(tuple, picks):
                lo, hi = base.copy(), base.copy()
                lo[idx] -= h
                hi[idx] += h
                args = {"features": (x, A, v), "adjs": (x, A, v), "vector": (x, A, v)}[name]
                args = tuple(b if b is not base else None for b in args)
                fd = (f(*(hi if a is None else a for a in args)) - f(*(lo if a is None else a for a in args))) / (2 * h)
                scale = max(np.abs(grads[name]).max(), 1e-12)
                if kind == "regression" and name == "adjs":
                    assert fd == 0.0 and grads[name][idx] == 0.0
                else:
                    assert abs(fd - grads[name][idx]) <= 1e-6 * scale + 1e-9, (kind, g, name, idx, fd, grads[name][idx])
        # the gradient at the first layer's output, which the closed form differentiates to
        y1 = IO.O.dense_bn_fwd(v[None], IO._first_layer(kind, P), "relu")[0]
        _, g1 = IO.score_grads(kind, P, x, A, None, mask, size, first=y1)
        for j in rng.permutation(y1.shape[0])[:8]:
            lo, hi = y1.copy(), y1.copy()
            lo[j] -= h
            hi[j] += h
            fd = (IO.score_grads(kind, P, x, A, None, mask, size, first=hi)[0] - IO.score_grads(kind, P, x, A, None, mask, size, first=lo)[0]) / (2 * h)
            assert abs(fd - g1["first"][j]) <= 1e-6 * np.abs(g1["first"]).max() + 1e-9


def test_the_regression_model_has_no_adjacency_gradient():
    for g in IO.COMPOUNDS:
        P, x, A, v, size = _compound("regression", g)
        for mask in (np.array([1.0, 0.0]), np.array([1.0, 1.0])):
            s, grads = IO.score_grads("regression", P, x, A, v, mask, size)
            assert not grads["adjs"].any()
            assert IO.score_grads("regression", P, x, A * 0.0, v, mask, size)[0] == s
    with pytest.raises(ValueError):
        IO.modal_targets("regression", "adjs")
    assert "adjs" not in IO.modal_targets("regression", "all")[0]


@pytest.mark.parametrize("kind", KINDS)
def test_relu_units_of_the_gpu_cases_stay_off_zero(kind):
    """For the parameter seeds, compounds, D, noise seed and noise scale the GPU tests use: no relu pre-activation of a copy with
    non-zero weight lies within 1e-5 of its layer's largest |pre| of zero, for any modal and method.  Nothing is excluded."""
    worst = np.inf
    for g in IO.COMPOUNDS:
        P, x, A, v, size = _compound(kind, g)
        for modal in _modals(kind):
            for method in IO.METHODS:
                m = IO.relu_margins(kind, P, x, A, v, np.array([1.0, 0.0]), modal, method, IO.DIVIDE, size, _noise(method, g, x, A, v),
                                    IO.NOISE_SCALE)
                assert m, (kind, modal, method)
                for layer, (lo, hi) in m.items():
                    worst = min(worst, lo / hi)
                    assert lo >= 1e-5 * hi, (kind, g, modal, method, layer, lo, hi)
    print("relu margin, %s (parameter seed %d): smallest |pre| / max |pre| = %.2e" % (kind, IO.PARAM_SEEDS[kind], worst))


def test_sweeps_of_the_oracle():
    rng = np.random.default_rng(3)
    Pm, bias = rng.standard_normal((2, 5)), rng.standard_normal(5)
    scale, shift = rng.random(5) + 0.5, rng.standard_normal(5)
    Y = IO.expand(Pm, [0.0, 0.5, 1.0], bias, scale, shift, "relu")
    assert Y.shape == (6, 5) and np.array_equal(Y[3], np.maximum(scale * bias + shift, 0.0))
    assert np.allclose(Y[5], np.maximum(scale * (Pm[1] + bias) + shift, 0.0), rtol=1e-15)
    dY = rng.standard_normal((6, 5))
    dY[[0, 3]] = np.nan                                             # the copies of weight 0
    S = IO.reduce(dY, Y, [0.0, 0.25, 0.75], scale, "relu")
    assert np.isfinite(S).all() and np.allclose(S[0], scale * (0.25 * dY[1] * (Y[1] > 0) + 0.75 * dY[2] * (Y[2] > 0)), rtol=1e-15)


# ---- the public function's refusals, on the host ------------------------------------------------------------------------------------------
def test_public_function_refuses_on_the_host():
    import kgcn  # noqa: F401  (the alias package resolves to the same modules)
    from kgcn_amd import models, visualization as V
    vec, reg = models.MultimodalVecGCN(1, 2), models.MultimodalRegressionGCN(2)
    x, A, v = Z["ds_feature"][:3], Z["ds_dense_adj"][:3], Z["ds_profeat"][:3]
    with pytest.raises(TypeError):
        V.vecmodal_integrated_gradients(models.GCN(1, 2), x, A, v)
    with pytest.raises(TypeError):
        V.vecmodal_ig_targets(object(), "all")
    with pytest.raises(ValueError):
        V.vecmodal_integrated_gradients(reg, x, A, v, modal="adjs")
    with pytest.raises(ValueError):
        V.vecmodal_integrated_gradients(vec, x, A, v, modal="embedded_layer")
    with pytest.raises(ValueError):
        V.vecmodal_integrated_gradients(vec, x, A, v, modal="dragon")          # the other model's vector
    with pytest.raises(ValueError):
        V.vecmodal_integrated_gradients(vec, x, A, v, vector_name="features")
    with pytest.raises(ValueError):
        V.vecmodal_integrated_gradients(vec, x, A, v, method="deeplift")
    with pytest.raises(ValueError):
        V.vecmodal_integrated_gradients(vec, x, A, v, divide_number=0)
    with pytest.raises(ValueError):
        V.vecmodal_integrated_gradients(vec, x, A, v, method="smooth_ig", noise_scale=-0.1)
    with pytest.raises(ValueError):
        V.vecmodal_integrated_gradients(vec, x, A, v, chunk=0)
    with pytest.raises(ValueError):
        V.vecmodal_integrated_gradients(vec, x, A, None)
    assert V.vecmodal_ig_targets(vec, "all") == (("features", "adjs", "profeat"), "profeat")
    assert V.vecmodal_ig_targets(reg, "all") == (("features", "dragon"), "dragon")
    assert V.vecmodal_ig_targets(reg, "descr", vector_name="descr") == (("descr",), "descr")
    assert V.vecmodal_ig_targets(vec, "adjs") == (("adjs",), "profeat")


def test_ops_limits_on_the_host():
    from kgcn_amd import ops
    assert ops.ig_copies_limits_check(0, 1, 1) == (0, 1, 1)
    assert ops.ig_copies_limits_check(5, ops.IG_COPIES_MAX_COPIES, ops.IG_COPIES_MAX_WIDTH) == (5, ops.IG_COPIES_MAX_COPIES, ops.IG_COPIES_MAX_WIDTH)
    for bad in ((1, 0, 8), (1, 2, 0), (1, ops.IG_COPIES_MAX_COPIES + 1, 8), (1, 2, ops.IG_COPIES_MAX_WIDTH + 1), (-1, 2, 8),
                (ops.IG_COPIES_MAX_ROWS // 2 + 1, 2, 8)):
        with pytest.raises(ValueError):
            ops.ig_copies_limits_check(*bad)
    assert ops.IG_STREAM_VECTOR not in (ops.IG_STREAM_FEATURES, ops.IG_STREAM_SEQUENCE)
    assert not ops.IG_STREAM_ADJACENCY <= ops.IG_STREAM_VECTOR < ops.IG_STREAM_SEQUENCE       # the adjacency channels' range
    assert IO.STREAM_VECTOR == ops.IG_STREAM_VECTOR
