"""tests/cpi_ig_oracle.py on the CPU: the analytic per-step gradients of the literal loop against central differences, the closed
form against the literal loop (1e-10) for every modal set, method and 1 / 2 channels, completeness, and the host-side copy
coefficients of visualization.cpi_ig_coefficients against the ones the oracle derives on its own."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cpi_ig_oracle as O  # noqa: E402

N, F, WD, T = 7, 5, 12, 3
MODALS = ("all", "features", "adjs")
METHODS = ("ig", "grad_prod", "grad")


def _case(channels, seed=0):
    rng = np.random.default_rng(seed + channels)
    x, dense = O.make_compounds(rng, [5], N, F, channels)
    params = O.make_params(rng, F, WD, T, channels)
    adjs = [d[0] for d in dense]
    assert np.abs(adjs[0] - adjs[0].T).sum() > 0                      # directed
    assert np.count_nonzero(adjs[0][0]) == 1 and adjs[0][0, 0] == 1   # node 0: its self loop only
    assert not adjs[0][5:].any() and not x[0, 5:].any()               # padded rows
    return params, x[0], adjs


@pytest.mark.parametrize("channels", [1, 2])
def test_literal_gradients_match_central_differences(channels):
    params, x, adjs = _case(channels)
    x = x.astype(np.float64)
    adjs = [a.astype(np.float64) for a in adjs]
    h = 1e-6
    for t in range(T):
        dx, dA0, p = O.grads(params, x, adjs, t)
        assert 0.0 < p < 1.0
        rng = np.random.default_rng(t)
        for _ in range(12):
            i, j = int(rng.integers(0, N)), int(rng.integers(0, F))
            xp, xm = x.copy(), x.copy()
            xp[i, j] += h
            xm[i, j] -= h
            fd = (O.forward(params, xp, adjs, t)[0] - O.forward(params, xm, adjs, t)[0]) / (2 * h)
            assert abs(fd - dx[i, j]) <= 1e-8 * max(1.0, np.abs(dx).max()), (t, i, j, fd, dx[i, j])
            i, j = int(rng.integers(0, N)), int(rng.integers(0, N))
            ap, am = [a.copy() for a in adjs], [a.copy() for a in adjs]
            ap[0][i, j] += h
            am[0][i, j] -= h
            fd = (O.forward(params, x, ap, t)[0] - O.forward(params, x, am, t)[0]) / (2 * h)
            assert abs(fd - dA0[i, j]) <= 1e-8 * max(1.0, np.abs(dA0).max()), (t, i, j, fd, dA0[i, j])


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("modal", MODALS)
def test_closed_form_equals_the_literal_loop(modal, method, channels):
    params, x, adjs = _case(channels)
    for t in (0, T - 1):
        lit = O.literal(params, x, adjs, t, modal, method, D=20)
        cf = O.closed_form(params, x, adjs, t, modal, method, D=20)
        assert set(lit) == set(cf)
        for k in lit:
            ref = np.asarray(lit[k], np.float64)
            assert np.abs(ref).max() > 0
            assert np.abs(np.asarray(cf[k]) - ref).max() <= 1e-10 * max(1.0, np.abs(ref).max()), (k, t)
        if "adjs_IG" in lit:                                          # nothing off the stored entries of channel 0
            assert not lit["adjs_IG"][adjs[0] == 0].any() and np.abs(lit["adjs_IG"]).max() > 0


@pytest.mark.parametrize("modal,channels", [("all", 1), ("features", 1), ("adjs", 1), ("features", 2)])
def test_completeness(modal, channels):
    """sum_of_IG -> end - start as D grows (a right Riemann sum: the gap falls like 1 / D).  The values of EVERY channel are
    scaled but only channel 0 is attributed, so with a second channel completeness holds for the features alone."""
    params, x, adjs = _case(channels)
    gaps = []
    for D in (10, 100, 1000):
        r = O.closed_form(params, x, adjs, 1, modal, "ig", D)
        gaps.append(abs(r["sum_of_IG"] - (r["end"] - r["start"])))
    assert abs(r["end"] - r["start"]) > 1e-3
    assert gaps[1] < gaps[0] / 5 and gaps[2] < gaps[1] / 5 and gaps[2] < 1e-2 * abs(r["end"] - r["start"]), gaps


@pytest.mark.parametrize("method,D", [("ig", 1), ("ig", 7), ("ig", 100), ("grad_prod", 100), ("grad", 100)])
@pytest.mark.parametrize("modal", MODALS)
def test_copy_coefficients_of_the_public_helper(modal, method, D):
    """alpha, gamma, wA, wB of the fused route, per modal set and method."""
    from kgcn_amd import visualization as V
    co = V.cpi_ig_coefficients(modal, method, D)
    targets, s, w, a, c = O.copy_coefficients(modal, method, D)
    assert tuple(co["targets"]) == tuple(targets)
    K = len(s)
    assert K == (D + 1 if method == "ig" else 2) and all(len(co[k]) == K for k in ("scales", "weights", "alpha", "gamma", "wA"))
    eq = lambda got, want: np.allclose(np.asarray(got, np.float64), want, rtol=1e-15, atol=0)
    assert eq(co["scales"], s) and eq(co["weights"], w)
    assert eq(co["alpha"], a * c) and eq(co["gamma"], c)
    # G^A carries beta = c for the features and beta = a for the Y0 term of the adjacency values; the bias term has beta = 1
    if "features" in targets:
        assert eq(co["wA"], w * c)
    if "adjs" in targets:
        assert eq(co["wA"], w * a)
        bias = co["wB"] if co["bias_from"] == "B" else co["wA"]
        assert eq(bias, w)
    assert (co["wB"] is None) == (modal != "all") and co["bias_from"] == ("B" if modal == "all" else "A")
    assert co["weights"][0] == 0.0 and co["scales"][0] == 0.0 and co["scales"][-1] == 1.0


def test_refusals_of_the_public_helper():
    from kgcn_amd import visualization as V
    with pytest.raises(ValueError):
        V.cpi_ig_coefficients("embedded_layer", "ig", 10)
    for method in ("smooth_grad", "smooth_ig"):
        with pytest.raises(ValueError):
            V.cpi_ig_coefficients("all", method, 10)
    with pytest.raises(ValueError):
        V.cpi_ig_coefficients("all", "ig", 0)


def test_sweep_matches_the_per_copy_gradients():
    """The op-level oracle: GA of sweep() contracted like a GraphConv backward is the weighted sum of grads() over the copies."""
    params, x, adjs = _case(2)
    x = x.astype(np.float64)
    W, b, _, _ = O._p64(params)
    targets, s, w, a, c = O.copy_coefficients("all", "ig", 6)
    P, Q, _ = O.products(params, x, adjs)
    heads = [O.task_head(params, t) for t in range(T)]
    p, GA, GB = O.sweep(P, Q, np.stack([h[0] for h in heads]), [h[1] for h in heads], a * c, c, w * c, w)
    for t in range(T):
        want = 0.0
        for k in range(len(s)):
            dx, _, pk = O.grads(params, x * a[k], [A * c[k] for A in adjs], t)
            assert abs(pk - p[k, t]) <= 1e-12
            want = want + w[k] * dx
        got = sum(np.asarray(A, np.float64).T @ GA[t] @ W[ch].T for ch, A in enumerate(adjs))
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
        assert np.abs(GB[t]).max() > 0


def test_binding_and_per_pass_cap_match_the_header():
    """ops.cpi_ig is bound, and the tasks-per-pass cap the GPU test sizes its T by is the one the kernel is compiled with."""
    import re
    from kgcn_amd import _lib, ops
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kgcn_hip.h")).read()
    assert int(re.search(r"#define\s+KGCN_CPIIG_TASKS_PER_PASS\s+(\d+)", header).group(1)) == ops.CPI_IG_TASKS_PER_PASS
    for name in ("kgcn_cpi_ig_f32", "kgcn_cpi_ig_workspace_bytes"):
        assert name in _lib.SIGNATURES, name
    assert _lib.lib.kgcn_cpi_ig_workspace_bytes(2, 512, 3, 101) == 2 * 101 * (512 + 3) * 4
    assert _lib.lib.kgcn_cpi_ig_workspace_bytes(0, 512, 3, 101) == 0
    # validation before any launch: status + message, no GPU needed
    assert _lib.lib.kgcn_cpi_ig_f32(None, None, 1, 4, 8, None, None, 1, None, None, None, None, 1, None, None, None, None, 0, None) != 0
    assert b"copies" in _lib.lib.kgcn_last_error()
    assert _lib.lib.kgcn_cpi_ig_f32(None, None, 1, 4, 8, None, None, 1, None, None, None, None, 2, None, None, None, None, 0, None) != 0
    assert b"NULL" in _lib.lib.kgcn_last_error()
    with pytest.raises(ValueError):
        ops.cpi_ig_limits_check(10, 512, 3, 1)
