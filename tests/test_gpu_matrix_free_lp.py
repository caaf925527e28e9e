"""Label propagation without a stored affinity matrix, and predict_proba, on the GPU (csrc/labelprop.hip through ops.rbf_apply /
rbf_degrees / lp_propagate_free and kgcn_amd/active_learning.py).  The matrix-free route is held to the stored route BIT FOR BIT:
every w_ij is rebuilt with the arithmetic of the affinity kernel and summed in the stored kernels' order, so the oracle
(tests/active_learning_oracle.py) applied to the device's own stored W is the reference, and everything recorded from scikit-learn
in tests/golden/g16_active_learning.npz applies unchanged.  predict_proba is held to what scikit-learn recorded in
tests/golden/g17_lp_predict.npz within ten times the distance measured on the GPU (g17_lp_predict_bounds.json)."""
import ctypes
import functools
import json
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import active_learning_cases as cases  # noqa: E402
import active_learning_oracle as O  # noqa: E402
import matrix_free_oracle as MO  # noqa: E402

PREDICT_CASES, case_parts, predict_fixture = MO.PREDICT_CASES, MO.case_parts, MO.predict_fixture

pytestmark = pytest.mark.gpu

# n: both sides of the 64-tile and of the 32-row block of the convergence partials, one and several workgroups; d: both sides of the
# MFMA's k-step of 4 and of the 16 attributes staged at a time; K: both sides of the 4- and the 8-column chunk, and the most there is
NS, DS, KS = (1, 31, 33, 64, 65, 129, 257), (1, 3, 16, 17, 33), (1, 4, 5, 8, 9, 64)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def points(n, d, seed):
    return np.random.default_rng(seed).standard_normal((n, d))


# ---- 1. rbf_apply on one set ---------------------------------------------------------------------------------------------------------
def one_set_case(X, gamma, K, seed):
    """rbf_apply over X itself against the oracle's product over the device's stored W, with and without the diagonal."""
    from kgcn_amd import ops
    n = X.shape[0]
    Xd = dev(X)
    W = ops.rbf_affinity(Xd, gamma).cpu().numpy()
    G = np.random.default_rng(seed).standard_normal((n, K))
    W0 = W.copy()
    np.fill_diagonal(W0, 0.0)
    for zero, Wref in ((False, W), (True, W0)):
        got = ops.rbf_apply(Xd, Xd, gamma, dev(G), same_set=True, zero_diagonal=zero).cpu().numpy()
        assert same_bits(got, O.product(Wref, G)), (n, X.shape[1], K, zero)


@pytest.mark.parametrize("n", NS)
def test_rbf_apply_on_one_set_is_the_stored_product(n):
    """Tiles below the diagonal are computed as b.a where the stored kernel mirrored a.b: the bits must not differ."""
    for d in DS:
        for K in KS:
            one_set_case(points(n, d, 100 * n + d), 1.0 / d, K, n + d + K)


def test_rbf_apply_duplicates_and_a_far_point():
    rng = np.random.default_rng(5)
    X = rng.integers(-8, 9, (70, 5)).astype(np.float64)
    X[[3, 40, 69]] = X[0]                                        # distance exactly 0 off the diagonal
    one_set_case(X, 0.125, 5, 1)
    Y = rng.standard_normal((66, 7)) * 1e3                       # duplicates whose norms round: the distance is clamped
    Y[[1, 65]] = Y[0]
    one_set_case(Y, 1e-7, 4, 2)
    Z = rng.standard_normal((65, 3))
    Z[64] = 1e3                                                  # a whole row of w underflows to 0
    one_set_case(Z, 0.5, 9, 3)
    from kgcn_amd import ops
    Zd = dev(Z)
    ones = dev(np.ones((65, 1)))
    assert ops.rbf_apply(Zd, Zd, 0.5, ones, same_set=True, zero_diagonal=True)[64].item() == 0.0
    assert ops.rbf_apply(Zd, Zd, 0.5, ones, same_set=True)[64].item() == 1.0


# ---- 2. rbf_apply between two sets ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", [(1, 65), (65, 1), (70, 130), (130, 70)])
def test_rbf_apply_rectangular_is_the_off_diagonal_block_of_the_union(m, n):
    from kgcn_amd import ops
    for d in DS:
        for K in (1, 5, 9):
            U = points(m + n, d, 1000 * m + n + d)
            U[m + n // 2] = U[0]                                 # a reference that IS a query: no diagonal rule between two sets
            W = ops.rbf_affinity(dev(U), 1.0 / d).cpu().numpy()[:m, m:]
            G = np.random.default_rng(K).standard_normal((n, K))
            got = ops.rbf_apply(dev(U[:m]), dev(U[m:]), 1.0 / d, dev(G)).cpu().numpy()
            assert same_bits(got, MO.product_rect(W, G)), (m, n, d, K)


# ---- 3. degrees ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_rbf_degrees_are_the_stored_degrees(n):
    from kgcn_amd import ops
    for d in DS:
        Xd = dev(points(n, d, 7 * n + d))
        s, dg = ops.lp_degrees(ops.rbf_affinity(Xd, 1.0 / d))
        fs, fd = ops.rbf_degrees(Xd, 1.0 / d)
        assert same_bits(fs.cpu().numpy(), s.cpu().numpy()) and same_bits(fd.cpu().numpy(), dg.cpu().numpy()), (n, d)


# ---- 4. propagation ------------------------------------------------------------------------------------------------------------------
def make_case(n, d, widths, seed, labelled=0.25):
    """Three blobs and a label matrix [n, len(widths)] of class indices (-1 = unlabelled); every task has a labelled row."""
    rng = np.random.default_rng(seed)
    cluster = rng.integers(0, 3, n)
    X = 2.0 * rng.standard_normal((3, d))[cluster] + rng.standard_normal((n, d))
    labels = np.stack([np.where(rng.random(n) < labelled, cluster % w, -1) for w in widths], axis=1).astype(np.int32)
    labels[0] = 0
    return X, labels, np.concatenate([[0], np.cumsum(widths)])


def both_routes(X, gamma, labels, task_col, variant, **kw):
    """-> ((dist, n_iter, status) of lp_propagate on the stored W, the same of lp_propagate_free), on the host."""
    from kgcn_amd import ops
    Xd, ld = dev(X), dev(labels)
    W = ops.rbf_affinity(Xd, gamma)
    out = []
    for sd, run in ((ops.lp_degrees(W), lambda scale: ops.lp_propagate(W, scale, ld, task_col, variant, **kw)),
                    (ops.rbf_degrees(Xd, gamma), lambda scale: ops.lp_propagate_free(Xd, gamma, scale, ld, task_col, variant, **kw))):
        r = run(sd[1] if variant == O.SPREADING else sd[0])
        out.append(tuple(t.cpu().numpy() for t in r[:3]) + (r[3],))
    return out


def assert_same_run(stored, free, what):
    assert np.array_equal(stored[1], free[1]) and np.array_equal(stored[2], free[2]), (what, stored[1:3], free[1:3])
    assert same_bits(stored[0], free[0]), what
    assert stored[3] == free[3], what


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("variant,alpha", [(O.PROPAGATION, 0.2), (O.SPREADING, 0.2), (O.SPREADING, 0.9)])
def test_lp_propagate_free_is_lp_propagate(n, variant, alpha):
    """Column counts 1, 4, 5, 8, 9 (one class a task, the 4-column chunk, the 8-column chunk and its two sides)."""
    for d, widths in ((1, (1,)), (3, (2, 2)), (16, (2, 3)), (17, (3, 3, 2)), (33, (3, 3, 3))):
        X, labels, task_col = make_case(n, d, widths, 7 * n + d)
        stored, free = both_routes(X, 0.5 / d, labels, task_col, variant, alpha=alpha, max_iter=40)
        assert_same_run(stored, free, (n, d, widths))


@pytest.mark.parametrize("variant", [O.PROPAGATION, O.SPREADING])
def test_lp_propagate_free_32_tasks_over_64_columns(variant):
    X, labels, task_col = make_case(129, 5, (2,) * 32, 11)
    stored, free = both_routes(X, 0.1, labels, task_col, variant, max_iter=25)
    assert_same_run(stored, free, "T = 32")
    assert free[0].shape == (129, 64)


@pytest.mark.parametrize("variant", [O.PROPAGATION, O.SPREADING])
def test_lp_propagate_free_frozen_tasks_and_the_check_interval(variant):
    """Task 0 has no unlabelled row: under propagation it converges at step 1 and is frozen while the others run into max_iter.
    With widths (8, 3) it fills the first 8-column chunk alone, which is then skipped; with the others its chunk is still
    multiplied for the tasks beside it."""
    n = 257
    for widths in ((2, 3, 2), (8, 3), (4, 2, 3)):
        X, labels, task_col = make_case(n, 3, widths, 11)
        labels[:, 0] = np.arange(n) % widths[0]
        stored, free = both_routes(X, 0.5, labels, task_col, variant, tol=1e-9, max_iter=5)
        assert_same_run(stored, free, widths)
        if variant == O.PROPAGATION:
            assert free[1].tolist() == [1] + [5] * (len(widths) - 1) and free[2][0] == O.CONVERGED and np.all(free[2][1:] == O.MAX_ITER)
        full = both_routes(X, 0.5, labels, task_col, variant)
        assert_same_run(full[0], full[1], widths)
        for ipc in (1, 3, 8):
            other = both_routes(X, 0.5, labels, task_col, variant, iters_per_check=ipc)
            assert_same_run(other[0], other[1], (widths, ipc))
            assert same_bits(other[1][0], full[1][0]) and np.array_equal(other[1][1], full[1][1])      # the interval changes no bit
        assert variant == O.SPREADING or len(set(full[1][1].tolist())) > 1                             # tasks stopped at different steps


@pytest.mark.parametrize("variant", [O.PROPAGATION, O.SPREADING])
def test_lp_propagate_free_isolated_point(variant):
    n = 65
    X, labels, task_col = make_case(n, 2, (2, 3), 4)
    X[-1] = 1e3
    labels[-1] = -1
    stored, free = both_routes(X, 0.5, labels, task_col, variant)
    assert_same_run(stored, free, "isolated")
    assert np.all(free[0][-1] == 0.0) and np.all(np.isfinite(free[0]))


# ---- 5. the drivers on the matrix-free route -----------------------------------------------------------------------------------------
def estimator(alg, gamma, z, matrix_free, **kw):
    from kgcn_amd import active_learning as al
    est = al.LabelSpreading(gamma=gamma, alpha=float(z["alpha"]), **kw) if alg == "LS" else al.LabelPropagation(gamma=gamma, **kw)
    est.matrix_free = matrix_free
    return est


@functools.lru_cache(None)
def fitted(tag, matrix_free):
    z = cases.fixture()
    key, n, d, gamma, alg, variant = cases.parts(tag)
    model = estimator(alg, gamma, z, matrix_free, max_iter=int(z["max_iter"]), tol=float(z["tol"]))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model.fit_tasks(z[key + "_X"], z[key + "_Y"])
    return model


@pytest.mark.parametrize("tag", cases.TAGS)
def test_fit_tasks_matrix_free_equals_the_stored_route_and_scikit_learn(tag):
    z, b = cases.fixture(), cases.bounds()["fits"][tag]
    free, stored = fitted(tag, True), fitted(tag, False)
    assert free.matrix_free_ is True and stored.matrix_free_ is False
    for a, c in zip(free.label_distributions_, stored.label_distributions_):
        assert same_bits(a, c)
    assert free.n_iter_.tolist() == stored.n_iter_.tolist() == z[tag + "_n_iter"].tolist()
    assert np.array_equal(free.status_, stored.status_)
    assert np.array_equal(np.stack(free.transduction_, axis=1), z[tag + "_transduction"])
    distance = float(np.abs(np.concatenate(free.label_distributions_, axis=1) - z[tag + "_dist"]).max())
    print("%s matrix-free: distance from scikit-learn %.3g (bound %.3g)" % (tag, distance, b["bound"]))
    assert distance <= b["bound"]


@pytest.mark.parametrize("tag", [t for t in cases.TAGS if "_g1d_" in t])
def test_selections_matrix_free_equal_the_recorded_ones(tag):
    from kgcn_amd import active_learning as al, ops
    z = cases.fixture()
    key, n, d, gamma, alg, variant = cases.parts(tag)
    X, Y = z[key + "_X"], z[key + "_Y"]
    kw = dict(algorithm=alg, gamma=gamma, alpha=float(z["alpha"]), tol=float(z["tol"]), matrix_free=True)
    assert al.query_next_data_points(X, Y, US_strategy="E", **kw).tolist() == z[tag + "_top5_E"].tolist()
    presence = ~(Y == -1).all(axis=1)
    for strat in ("LC", "MS"):
        got = al.query_next_data_points(X, Y[:, [0, 2]], label_presence=presence, US_strategy=strat, **kw)
        assert got.tolist() == z["%s_top5_%s" % (tag, strat)].tolist(), strat
    unl = cases.unlabeled(key)
    dist = dev(np.concatenate(fitted(tag, True).label_distributions_, axis=1))
    sc = ops.lp_scores(dist, cases.TASK_COL, dev(unl.astype(np.int32)))
    for strat, row, largest in (("E", "E", True), ("LC", "LC_TASKS", False), ("MS", "MS_TASKS", False)):
        pick = ops.lp_select(sc[O.SCORES[row]], dev(unl.astype(np.int32)), n, 1, largest).item()
        assert unl[pick] == z["%s_pick_%s" % (tag, strat)][0], strat


@pytest.mark.parametrize("tag", cases.LOOP_TAGS)
@pytest.mark.parametrize("strategy", ["E", "LC", "MS"])
def test_query_and_teach_matrix_free_equals_the_recorded_loops(tag, strategy):
    from kgcn_amd import active_learning as al
    z = cases.fixture()
    key, n, d, gamma, alg, variant = cases.parts(tag)
    m = int(z["loop_train"])
    X, truth = z[key + "_X"], z[key + "_truth"]
    for reuse in (True, False):
        learner = al.ActiveLearner(estimator(alg, gamma, z, True), X[:m], truth[:m], query_strategy=strategy)
        picks = learner.query_and_teach_n_times(10, X[m:], truth[m:], reuse=reuse)
        assert picks == z["%s_loop_%s" % (tag, strategy)].tolist(), reuse
    learner = al.ActiveLearner(estimator(alg, gamma, z, True), X[:m], truth[:m], query_strategy=strategy)
    assert learner.query(X[m:])[0] == z["%s_loop_%s" % (tag, strategy)][0]


# ---- 6. memory limits ----------------------------------------------------------------------------------------------------------------
def test_max_bytes_refuses_the_stored_route_and_auto_goes_matrix_free():
    from kgcn_amd import _lib, active_learning as al
    z = cases.fixture()
    X, Y, n = z["n65_X"], z["n65_Y"], 65
    want = fitted("n65_g1d_LP", False)

    def fit(matrix_free, max_bytes):
        est = estimator("LP", 1.0 / 3, z, matrix_free, max_iter=int(z["max_iter"]), tol=float(z["tol"]))
        est.max_bytes = max_bytes
        return est.fit_tasks(X, Y)
    with pytest.raises(_lib.KgcnHipError, match="max_bytes"):
        fit(False, n * n * 8 - 1)
    for mf, room, free in (("auto", n * n * 8 - 1, True), ("auto", n * n * 8, False), (True, n * n * 8, True), (False, n * n * 8, False)):
        got = fit(mf, room)
        assert got.matrix_free_ is free, (mf, room)
        for a, c in zip(got.label_distributions_, want.label_distributions_):
            assert same_bits(a, c)
    Xd = dev(X)
    small, roomy = al._Graph(Xd, 1.0 / 3, n * n * 8 - 1, "auto"), al._Graph(Xd, 1.0 / 3, n * n * 8, "auto")
    assert small.W is None and roomy.W is not None and tuple(roomy.W.shape) == (n, n)
    assert al._Graph(Xd, 1.0 / 3, None, True).W is None
    assert same_bits(small.s.cpu().numpy(), roomy.s.cpu().numpy()) and same_bits(small.d.cpu().numpy(), roomy.d.cpu().numpy())


# ---- 7. no n x n buffer --------------------------------------------------------------------------------------------------------------
def test_matrix_free_fit_allocates_no_n_by_n_buffer():
    import torch
    n, d = 4096, 8
    X, labels, _ = make_case(n, d, (2, 3, 2), 3)
    z = cases.fixture()
    est = estimator("LS", 1.0 / d, z, True, max_iter=20)
    Xd = dev(X)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        est.fit_tasks(Xd, labels)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print("matrix-free fit of %d points: %d bytes at the peak; W would take %d" % (n, peak, n * n * 8))
    assert n * n * 8 == 134217728 and peak < n * n * 8 // 8
    assert est.matrix_free_ is True and sum(p.shape[1] for p in est.label_distributions_) == 7


# ---- 8. prediction -------------------------------------------------------------------------------------------------------------------
def predict_bounds():
    with open(os.path.join(ROOT, "tests", "golden", "g17_lp_predict_bounds.json")) as f:
        return json.load(f)


@functools.lru_cache(None)
def fitted_single(case, matrix_free):
    z = cases.fixture()
    tag, key, gamma, alg, col = case_parts(case)
    model = estimator(alg, gamma, z, matrix_free, max_iter=int(z["max_iter"]), tol=float(z["tol"]))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return model.fit(z[key + "_X"], z[key + "_Y"][:, col])


def predict_distance(case):
    """The checks of one case; -> max |predict_proba - scikit-learn's| over its rows that are not NaN."""
    p = predict_fixture()
    tag, key, gamma, alg, col = case_parts(case)
    Xq, truth = p[key + "_Xq"], p[key + "_truthq"][:, col]
    free, stored = fitted_single(case, True), fitted_single(case, False)
    got, want = free.predict_proba(Xq), p[case + "_proba"]
    assert same_bits(got, stored.predict_proba(Xq))                 # both routes, equal bits
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got[-1]).all()
    assert np.array_equal(free.predict(Xq), p[case + "_predict"]) and free.predict(Xq)[-1] == free.classes_[0]
    assert free.score(Xq, truth) == float(p[case + "_score"]) == stored.score(Xq, truth)
    tasks = fitted(tag, True).predict_proba_tasks(Xq)               # one product over the 7 columns serves the three tasks
    assert len(tasks) == 3 and same_bits(tasks[col], got)
    assert same_bits(free.predict_proba_tasks(Xq)[0], got)
    return float(np.nanmax(np.abs(got - want)))


@pytest.mark.parametrize("case", PREDICT_CASES)
def test_prediction_against_scikit_learn_within_the_recorded_bound(case):
    b = predict_bounds()
    distance = predict_distance(case)
    print("%s: predict_proba distance from scikit-learn %.17g (recorded %.17g, bound %.3g)" % (case, distance, b["distance"], b["bound"]))
    assert b["bound"] == 10.0 * b["distance"] and 0.0 < b["distance"] < 1e-12
    assert distance <= b["bound"]


def test_predict_proba_after_fit_tasks_needs_the_task_form():
    from kgcn_amd import active_learning as al
    Xq = predict_fixture()["n65_Xq"]
    with pytest.raises(al.NotFittedError, match="fit"):
        fitted("n65_g1d_LP", True).predict_proba(Xq)
    with pytest.raises(ValueError, match="attributes"):
        fitted("n65_g1d_LP", True).predict_proba_tasks(np.zeros((2, 5)))


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_before_any_launch():
    import torch
    from kgcn_amd import _lib, ops
    lib, ptr, stream = _lib.lib, _lib.ptr, _lib.current_stream
    n, d, K = 40, 4, 3
    X, G = dev(np.zeros((n, d))), dev(np.ones((n, K)))
    labels = dev(np.zeros((n, 1), np.int32))
    s, dg = ops.rbf_degrees(X, 1.0)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        for call in (lambda: ops.rbf_apply(X, X, bad, G, same_set=True), lambda: ops.rbf_degrees(X, bad),
                     lambda: ops.lp_propagate_free(X, bad, s, labels, [0, 2], O.PROPAGATION)):
            with pytest.raises(_lib.KgcnHipError, match="gamma"):
                call()
    for bad in (np.nan, np.inf):
        Xb = np.zeros((n, d))
        Xb[3, 1] = bad
        Xb = dev(Xb)
        for call in (lambda: ops.rbf_apply(Xb, Xb, 1.0, G, same_set=True), lambda: ops.rbf_apply(Xb, X, 1.0, G),
                     lambda: ops.rbf_apply(X, Xb, 1.0, G), lambda: ops.rbf_degrees(Xb, 1.0),
                     lambda: ops.lp_propagate_free(Xb, 1.0, s, labels, [0, 2], O.PROPAGATION)):
            with pytest.raises(_lib.KgcnHipError, match="not finite"):
                call()
    empty = torch.empty((n, 0), device="cuda", dtype=torch.float64)
    wide = torch.ones((n, ops.LP_MAX_COLS + 1), device="cuda", dtype=torch.float64)
    for call in (lambda: ops.rbf_degrees(empty, 1.0), lambda: ops.rbf_apply(empty, empty, 1.0, G, same_set=True),
                 lambda: ops.rbf_apply(X, X, 1.0, wide, same_set=True), lambda: ops.rbf_apply(X, X[:, :2].contiguous(), 1.0, G),
                 lambda: ops.lp_propagate_free(empty, 1.0, s, labels, [0, 2], O.PROPAGATION)):
        with pytest.raises(_lib.KgcnHipError, match="shape"):
            call()
    with pytest.raises(ValueError, match="zero_diagonal"):
        ops.rbf_apply(X, X.clone(), 1.0, G, zero_diagonal=True)
    # the library's own checks, through the raw ABI: a status, a message, and nothing written
    out = torch.full((n, K), -7.0, device="cuda", dtype=torch.float64)
    norms = torch.full((2, n), -7.0, device="cuda", dtype=torch.float64)
    deg = torch.full((2, n), -7.0, device="cuda", dtype=torch.float64)
    one, zero = ctypes.byref(ctypes.c_double(1.0)), ctypes.byref(ctypes.c_double(0.0))
    big = ops.LP_MAX_ROWS + 1

    def apply(n_=n, d_=d, g=one, cols=K, xq=X, same=1, zd=0):
        return lib.kgcn_rbf_apply_f64(ptr(xq), n_, ptr(X), n_, d_, g, ptr(G), cols, same, zd, ptr(out), ptr(norms[0]), ptr(norms[1]), stream())

    def degrees(n_=n, d_=d, g=one, x=X):
        return lib.kgcn_rbf_degrees_f64(ptr(x), n_, d_, g, ptr(deg[0]), ptr(deg[1]), ptr(norms[0]), stream())
    for kw, word in ((dict(d_=0), b"attributes"), (dict(n_=big), b"points"), (dict(n_=0), b"points"), (dict(g=zero), b"gamma"),
                     (dict(g=None), b"gamma"), (dict(cols=ops.LP_MAX_COLS + 1), b"columns"), (dict(cols=0), b"columns"),
                     (dict(xq=None), b"NULL"), (dict(same=0, zd=1), b"zero_diagonal"), (dict(xq=G), b"same_set")):
        assert apply(**kw) != 0 and word in lib.kgcn_last_error(), (kw, lib.kgcn_last_error())
    for kw, word in ((dict(d_=0), b"attributes"), (dict(n_=big), b"points"), (dict(g=zero), b"gamma"), (dict(x=None), b"NULL")):
        assert degrees(**kw) != 0 and word in lib.kgcn_last_error(), (kw, lib.kgcn_last_error())
    T, Kc = 1, 2
    need = lib.kgcn_lp_workspace_bytes(n, T, Kc)
    ws = torch.zeros((need,), device="cuda", dtype=torch.uint8)
    meta = torch.full((2, T), -7, device="cuda", dtype=torch.int32)
    tc = dev(np.array([0, 2], np.int32))

    def propagate(n_=n, d_=d, g=one, x=X, wsb=need, nrm=norms):
        return lib.kgcn_lp_propagate_free_f64(ptr(x), d_, g, ptr(nrm), ptr(s), n_, ptr(labels), ptr(tc), T, Kc, ops.LP_PROPAGATION, one, one,
                                              10, 0, 2, ptr(meta[0]), ptr(meta[1]), ptr(ws), wsb, stream())
    for kw, word in ((dict(wsb=need - 1), b"workspace"), (dict(d_=0), b"attributes"), (dict(n_=big), b"rows"), (dict(g=zero), b"gamma"),
                     (dict(x=None), b"NULL"), (dict(nrm=None), b"NULL")):
        assert propagate(**kw) != 0 and word in lib.kgcn_last_error(), (kw, lib.kgcn_last_error())
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((norms == -7.0).all()) and bool((deg == -7.0).all())
    assert bool((meta == -7).all()) and bool((ws == 0).all())
    assert propagate() == 0 and apply() == 0 and degrees() == 0                 # the same calls, well-formed, run
    torch.cuda.synchronize()
    assert bool((out == float(n)).all()) and bool((deg[0] == float(n)).all()) and bool((deg[1] == float(n - 1)).all())      # n coincident points
