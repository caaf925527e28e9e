"""The active-learning kernels on the GPU (csrc/labelprop.hip through kgcn_amd/ops.py rbf_affinity / lp_degrees / lp_propagate /
lp_scores / lp_select and kgcn_amd/active_learning.py).  The affinity matrix and the scores are held to the numpy oracle
(tests/active_learning_oracle.py) within ten times the distance measured on the GPU and recorded in the "gpu" section of
tests/golden/g16_active_learning_bounds.json; degrees, propagation and finish are the oracle's bit for bit given the device's own
W; the drivers are held to what scikit-learn recorded in tests/golden/g16_active_learning.npz within that file's bounds."""
import functools
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

pytestmark = pytest.mark.gpu

# A relative distance of W beyond this on standardised points is a finding about the kernel, not a bound to record: the squared
# distance carries a few roundings of |x_i|^2 + |x_j|^2 (relative 2^-53 each), exp one more.
AFFINITY_FINDING = 2.0 ** -48


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def gpu_bounds():
    return cases.bounds()["gpu"]


def affinity_distance(Wg, X, gamma):
    """max |W - oracle| / (oracle (1 + gamma (|x_i|^2 + |x_j|^2))): the rounding of the squared distance, which the norms scale and
    exp turns into a relative error of gamma times it, counted in the units it arises in.  Entries below 1e-290 count absolutely."""
    Wo = O.rbf_affinity(X, gamma)
    norms = (X * X).sum(axis=1)
    scale = np.maximum(Wo, 1e-290) * (1.0 + gamma * (norms[:, None] + norms[None, :]))
    return float((np.abs(Wg - Wo) / scale).max())


def affinity(X, gamma, **kw):
    from kgcn_amd import ops
    return ops.rbf_affinity(dev(X), gamma, **kw).cpu().numpy()


# ---- affinity --------------------------------------------------------------------------------------------------------------------
# n: both sides of the 16-row MFMA block and of the 64-row tile; d: both sides of the k-step of 4 and of the 16 attributes staged at a time
AFFINITY_N, AFFINITY_D = (1, 2, 15, 16, 17, 63, 64, 65, 257), (1, 3, 4, 5, 15, 16, 17, 33)


def affinity_case_distance(n):
    """The distance over the attribute counts of AFFINITY_D at n standard-normal points, gamma = 1 / d (what the recorded
    affinity_distance is the maximum of, together with rounded_duplicates_distance)."""
    worst = 0.0
    for d in AFFINITY_D:
        X = np.random.default_rng(n * 100 + d).standard_normal((n, d))
        W = affinity(X, 1.0 / d)
        assert W.shape == (n, n) and np.array_equal(bits(W), bits(W.T)) and np.all(np.diag(W) == 1.0)
        worst = max(worst, affinity_distance(W, X, 1.0 / d))
    return worst


@pytest.mark.parametrize("n", AFFINITY_N)
def test_affinity_both_sides_of_the_tile_and_of_the_k_step(n):
    worst = affinity_case_distance(n)
    print("affinity n = %d: distance %.3g (recorded %.3g, bound %.3g)" % (n, worst, gpu_bounds()["affinity_distance"],
                                                                          gpu_bounds()["affinity_bound"]))
    assert worst <= gpu_bounds()["affinity_bound"]


def test_affinity_recorded_distance_is_no_finding():
    g = gpu_bounds()
    assert g["affinity_bound"] == 10.0 * g["affinity_distance"] and 0.0 < g["affinity_distance"] <= AFFINITY_FINDING
    assert g["score_bound"] == 10.0 * g["score_distance"] and 0.0 < g["score_distance"] < 1e-13


def rounded_duplicates_distance():
    """Duplicates whose norms round: the squared distance may come out negative and is clamped."""
    Y = np.random.default_rng(6).standard_normal((66, 7)) * 1e3
    Y[[1, 65]] = Y[0]
    W = affinity(Y, 1e-7)
    assert np.all(W <= 1.0) and np.all(W[np.ix_([0, 1, 65], [0, 1, 65])] >= 1.0 - 1e-7 * 64 * 7e6 * 2.0 ** -52)
    return affinity_distance(W, Y, 1e-7)


def test_affinity_duplicates_and_a_far_point():
    rng = np.random.default_rng(5)
    X = rng.integers(-8, 9, (70, 5)).astype(np.float64)          # small integers: every product and sum is exact
    X[[3, 40, 69]] = X[0]
    W = affinity(X, 0.125)
    assert np.all(W[np.ix_([0, 3, 40, 69], [0, 3, 40, 69])] == 1.0)          # distance exactly 0 off the diagonal
    assert np.array_equal(bits(W), bits(O.rbf_affinity(X, 0.125))) or affinity_distance(W, X, 0.125) <= gpu_bounds()["affinity_bound"]
    assert rounded_duplicates_distance() <= gpu_bounds()["affinity_bound"]
    Z = rng.standard_normal((65, 3))
    Z[64] = 1e3                                                  # exp(-0.5 * ~3e6) underflows to 0
    W = affinity(Z, 0.5)
    assert np.all(W[64, :64] == 0.0) and np.all(W[:64, 64] == 0.0) and W[64, 64] == 1.0
    assert np.array_equal(bits(W), bits(W.T))


def test_affinity_refusals_before_any_launch():
    import torch
    from kgcn_amd import _lib, ops
    X = dev(np.zeros((100, 4)))
    with pytest.raises(_lib.KgcnHipError, match="max_bytes"):
        ops.rbf_affinity(X, 1.0, max_bytes=100 * 100 * 8 - 1)
    assert ops.rbf_affinity(X, 1.0, max_bytes=100 * 100 * 8).shape == (100, 100)
    W = torch.full((100, 100), -7.0, device="cuda", dtype=torch.float64)       # the library's own check: nothing is written
    import ctypes
    rc = _lib.lib.kgcn_rbf_affinity_f64(_lib.ptr(X), 100, 4, ctypes.byref(ctypes.c_double(1.0)), 79999, _lib.ptr(W), _lib.ptr(W[0]),
                                        _lib.current_stream())
    torch.cuda.synchronize()
    assert rc != 0 and b"max_bytes" in _lib.lib.kgcn_last_error() and bool((W == -7.0).all())
    for bad in (np.nan, np.inf):
        Xb = np.zeros((5, 2))
        Xb[3, 1] = bad
        with pytest.raises(_lib.KgcnHipError, match="not finite"):
            ops.rbf_affinity(dev(Xb), 1.0)
    with pytest.raises(_lib.KgcnHipError, match="gamma"):
        ops.rbf_affinity(X, 0.0)


# ---- degrees, propagation, finish: bits ------------------------------------------------------------------------------------------
def make_case(n, widths, seed, labelled=0.25):
    """Three blobs in the plane and a label matrix [n, len(widths)] of class indices: a task of `w` classes labels about a quarter of
    its rows (cluster index mod w), independently of the other tasks, so rows are labelled in one task and -1 in another."""
    rng = np.random.default_rng(seed)
    cluster = rng.integers(0, 3, n)
    X = 2.0 * rng.standard_normal((3, 2))[cluster] + rng.standard_normal((n, 2))
    labels = np.stack([np.where(rng.random(n) < labelled, cluster % w, -1) for w in widths], axis=1).astype(np.int32)
    labels[0] = 0                                                # every task has a labelled row
    return X, labels, np.concatenate([[0], np.cumsum(widths)])


@functools.lru_cache(None)
def device_graph(n, seed, gamma=0.5, far=False):
    """(X, W on the device, W on the host, (s, d) on the device) of make_case's points; far: the last point is isolated."""
    from kgcn_amd import ops
    X = make_case(n, (2,), seed)[0]
    if far:
        X[-1] = 1e3
    Wd = ops.rbf_affinity(dev(X), gamma)
    return X, Wd, Wd.cpu().numpy(), ops.lp_degrees(Wd)


def run(Wd, sd, labels, task_col, variant, alpha=0.2, tol=1e-3, max_iter=1000, ipc=None):
    from kgcn_amd import ops
    dist, n_iter, status, reads = ops.lp_propagate(Wd, sd[1] if variant == O.SPREADING else sd[0], dev(labels), task_col, variant,
                                                   alpha=alpha, tol=tol, max_iter=max_iter, iters_per_check=ipc)
    return dist.cpu().numpy(), n_iter.cpu().numpy(), status.cpu().numpy(), reads


def oracle_run(W, labels, task_col, variant, alpha=0.2, tol=1e-3, max_iter=1000):
    s, d = O.degrees(W)
    r = O.propagate(W, d if variant == O.SPREADING else s, labels, task_col, variant, alpha, tol, max_iter)
    return O.finish(r["F"], task_col), r["n_iter"], r["status"]


# 7 / 8 / 9: a wave of the step carries 8 rows; 31 / 32 / 33: its workgroup owns 32 (one convergence partial); 63 / 64 / 65: a lane
# owns the columns j = l mod 64
BIT_N = [2, 3, 7, 8, 9, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1025]


@pytest.mark.parametrize("n", BIT_N)
def test_degrees_are_the_oracles_bits(n):
    X, Wd, W, sd = device_graph(n, n)
    s, d = O.degrees(W)
    assert np.array_equal(bits(sd[0].cpu().numpy()), bits(s)) and np.array_equal(bits(sd[1].cpu().numpy()), bits(d))


@pytest.mark.parametrize("n", BIT_N)
@pytest.mark.parametrize("variant,alpha", [(O.PROPAGATION, 0.2), (O.SPREADING, 0.2), (O.SPREADING, 0.99)])
def test_propagation_and_finish_are_the_oracles_bits(n, variant, alpha):
    """T = 3 with one, two and three classes (six columns: the 8-column step), T = 1 with three classes (the 4-column step), and
    three tasks of three classes (nine columns: two passes of the 8-column step); to convergence or into max_iter."""
    X, Wd, W, sd = device_graph(n, n)
    cap = 1000 if n <= 257 and alpha < 0.9 else 12               # the oracle's cost; alpha = 0.99 converges slowly
    for widths in ((1, 2, 3), (3,), (3, 3, 3)):
        _, labels, task_col = make_case(n, widths, 7 * n + len(widths))
        got = run(Wd, sd, labels, task_col, variant, alpha, max_iter=cap)
        want = oracle_run(W, labels, task_col, variant, alpha, max_iter=cap)
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (widths, got[1:3], want[1:])
        assert np.array_equal(bits(got[0]), bits(want[0])), widths
        if n >= 31 and alpha < 0.9 and cap == 1000:
            assert np.all(got[2] == O.CONVERGED) and got[1].max() > 1


@pytest.mark.parametrize("variant", [O.PROPAGATION, O.SPREADING])
def test_frozen_tasks_keep_their_bits_and_the_check_interval_changes_nothing(variant):
    n = 257
    X, Wd, W, sd = device_graph(n, n)
    _, labels, task_col = make_case(n, (2, 3, 2), 11)
    labels[:, 0] = np.arange(n) % 2                              # task 0 has no unlabelled row
    tol = 1e-3 if variant == O.PROPAGATION else 1e-9
    base = run(Wd, sd, labels, task_col, variant, tol=tol, max_iter=5)
    want = oracle_run(W, labels, task_col, variant, tol=tol, max_iter=5)
    assert np.array_equal(bits(base[0]), bits(want[0])) and np.array_equal(base[1], want[1]) and np.array_equal(base[2], want[2])
    if variant == O.PROPAGATION:                                 # every row clamped: F' = F after the first step
        assert base[1].tolist() == [1, 5, 5] and base[2].tolist() == [O.CONVERGED, O.MAX_ITER, O.MAX_ITER]
        one = run(Wd, sd, labels, task_col, variant, tol=tol, max_iter=1)
        assert np.array_equal(bits(one[0][:, :2]), bits(base[0][:, :2]))       # frozen at step 1 beside tasks that ran four more
    else:
        assert base[1].tolist() == [5, 5, 5] and np.all(base[2] == O.MAX_ITER)
    full = run(Wd, sd, labels, task_col, variant)
    for ipc in (1, 7):
        other = run(Wd, sd, labels, task_col, variant, ipc=ipc)
        assert np.array_equal(bits(other[0]), bits(full[0])) and np.array_equal(other[1], full[1]) and np.array_equal(other[2], full[2])
    # one word is read back per iters_per_check steps, and none after the last task has stopped
    assert run(Wd, sd, labels, task_col, variant, ipc=1)[3] == int(full[1].max()) and full[3] == -(-int(full[1].max()) // 8)
    assert variant == O.SPREADING or len(set(full[1].tolist())) == 3          # propagation: the tasks stopped at three different steps


@pytest.mark.parametrize("variant", [O.PROPAGATION, O.SPREADING])
def test_an_isolated_point_gets_an_all_zero_row(variant):
    n = 65
    X, Wd, W, sd = device_graph(n, 3, far=True)
    assert sd[1][-1].item() == 0.0 and sd[0][-1].item() == 1.0
    _, labels, task_col = make_case(n, (2, 3), 4)
    labels[-1] = -1
    got = run(Wd, sd, labels, task_col, variant)
    want = oracle_run(W, labels, task_col, variant)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1])
    assert np.all(got[0][-1] == 0.0) and np.all(np.isfinite(got[0]))
    from kgcn_amd import ops
    sc = ops.lp_scores(dev(got[0]), task_col, dev(np.array([n - 1, 0], np.int32))).cpu().numpy()
    assert np.isnan(sc[O.SCORES["E"], 0]) and np.isfinite(sc[O.SCORES["E"], 1]) and np.all(sc[3:, 0] == 0.0)


# ---- scores and selection ----------------------------------------------------------------------------------------------------------
def scores_distance():
    from kgcn_amd import ops
    worst = 0.0
    for widths in ((2, 3, 2), (2, 2), (1, 3), (3,)):
        n = 300
        X, Wd, W, sd = device_graph(n, 21, far=True)
        _, labels, task_col = make_case(n, widths, 5)
        labels[-1] = -1
        dist = run(Wd, sd, labels, task_col, O.SPREADING)[0]
        cand = np.random.default_rng(1).permutation(n - 1)[:200].astype(np.int32)
        cand[7] = n - 1                                          # the zero row
        got, want = ops.lp_scores(dev(dist), task_col, dev(cand)).cpu().numpy(), O.scores(dist, task_col, cand)
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got[O.SCORES["E"], 7])
        worst = max(worst, float(np.nanmax(np.abs(got - want))))
        order = O.select(want[O.SCORES["E"]], 5, True)           # NaN is ordered last: the zero row is the very last entry
        assert order[-1] == 7
        assert ops.lp_select(dev(got[O.SCORES["E"]]), dev(cand), n, 5, True).cpu().numpy()[-1] == 7
    return worst


def test_scores_within_the_recorded_bound_of_the_oracle():
    worst = scores_distance()
    print("scores: distance %.3g (recorded %.3g, bound %.3g)" % (worst, gpu_bounds()["score_distance"], gpu_bounds()["score_bound"]))
    assert worst <= gpu_bounds()["score_bound"]


def test_exact_ties_follow_the_stated_rule():
    """Rows with equal distributions score equally in every strategy: the picks are those of a stable ascending sort, NaN last."""
    from kgcn_amd import ops
    rows = np.array([[0.5, 0.5, 0.25, 0.75], [0.9, 0.1, 0.6, 0.4], [0.0, 0.0, 0.5, 0.5], [0.75, 0.25, 0.5, 0.5]])
    dist = rows[[0, 1, 0, 3, 1, 0, 2, 3, 1, 0, 2, 1]]            # exact copies
    task_col, n = np.array([0, 2, 4]), 12
    cand = np.arange(n, dtype=np.int32)
    got, want = ops.lp_scores(dev(dist), task_col, dev(cand)).cpu().numpy(), O.scores(dist, task_col, cand)
    for row in range(5):
        for k, largest in ((5, True), (5, False), (1, True), (1, False), (8, True)):
            pick = ops.lp_select(dev(got[row]), dev(cand), n, k, largest).cpu().numpy()
            assert pick.tolist() == O.select(want[row], k, largest).tolist(), (row, k, largest)
    assert ops.lp_select(dev(got[0]), dev(cand), n, 1, True).item() == 10       # E: the LAST of the NaN rows
    assert ops.lp_select(dev(got[3]), dev(cand), n, 1, False).item() == 6       # LC: the FIRST among the equal minima (np.argmin)
    active = np.ones(n, np.int32)
    active[[10, 6, 0]] = 0
    for row, largest in ((0, True), (3, False), (4, False)):
        pick = ops.lp_select(dev(got[row]), dev(cand), n, 5, largest, active=dev(active)).cpu().numpy()
        assert pick.tolist() == O.select(want[row], 5, largest, active != 0).tolist()
    few = ops.lp_select(dev(got[0][:3].copy()), dev(cand[:3].copy()), n, 5, False).cpu().numpy()
    assert few.tolist() == O.select(want[0][:3], 5, False).tolist() + [-1, -1]


# ---- end to end --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def fitted(tag):
    from kgcn_amd import active_learning as al
    z = cases.fixture()
    key, n, d, gamma, alg, variant = cases.parts(tag)
    kw = dict(gamma=gamma, max_iter=int(z["max_iter"]), tol=float(z["tol"]))
    model = al.LabelSpreading(alpha=float(z["alpha"]), **kw) if alg == "LS" else al.LabelPropagation(**kw)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        model.fit_tasks(z[key + "_X"], z[key + "_Y"])
    return model, [w for w in caught if issubclass(w.category, al.ConvergenceWarning)]


@pytest.mark.parametrize("tag", cases.TAGS)
def test_fit_tasks_against_scikit_learn_within_the_recorded_bounds(tag):
    z, b = cases.fixture(), cases.bounds()["fits"][tag]
    model, caught = fitted(tag)
    dist = np.concatenate(model.label_distributions_, axis=1)
    distance = float(np.abs(dist - z[tag + "_dist"]).max())
    print("%s: distance from scikit-learn %.3g (the oracle's %.3g, bound %.3g), n_iter %s" % (tag, distance, b["distance"], b["bound"],
                                                                                            model.n_iter_.tolist()))
    assert model.n_iter_.tolist() == z[tag + "_n_iter"].tolist()
    assert np.array_equal(np.concatenate(model.classes_), z[tag + "_classes"])
    assert np.array_equal(np.stack(model.transduction_, axis=1), z[tag + "_transduction"])
    assert (len(caught) == 1) == (max(b["n_iter"]) == int(z["max_iter"]))          # scikit-learn's warning, and no exception
    assert distance <= b["bound"]


def test_fit_is_scikit_learns_single_task_interface():
    from kgcn_amd import active_learning as al
    z, tag = cases.fixture(), "n65_g1d_LS"
    m = al.LabelSpreading(gamma=1.0 / 3, alpha=float(z["alpha"])).fit(z["n65_X"], z["n65_Y"][:, 1])
    assert m.label_distributions_.shape == (65, 3) and m.classes_.tolist() == [3, 4, 5] and m.n_iter_ == int(z[tag + "_n_iter"][1])
    assert np.array_equal(m.transduction_, z[tag + "_transduction"][:, 1])
    assert np.array_equal(bits(m.label_distributions_), bits(fitted(tag)[0].label_distributions_[1]))     # one matrix served three tasks


@pytest.mark.parametrize("tag", [t for t in cases.TAGS if "_g1d_" in t])
def test_selections_equal_the_recorded_ones(tag):
    from kgcn_amd import active_learning as al, ops
    z = cases.fixture()
    key, n, d, gamma, alg, variant = cases.parts(tag)
    X, Y = z[key + "_X"], z[key + "_Y"]
    kw = dict(algorithm=alg, gamma=gamma, alpha=float(z["alpha"]), tol=float(z["tol"]))
    assert al.query_next_data_points(X, Y, US_strategy="E", **kw).tolist() == z[tag + "_top5_E"].tolist()
    presence = ~(Y == -1).all(axis=1)                            # the same rows, named by label_presence
    for strat in ("LC", "MS"):
        got = al.query_next_data_points(X, Y[:, [0, 2]], label_presence=presence, US_strategy=strat, **kw)
        assert got.tolist() == z["%s_top5_%s" % (tag, strat)].tolist(), strat
    unl = cases.unlabeled(key)
    dist = dev(np.concatenate(fitted(tag)[0].label_distributions_, axis=1))
    sc = ops.lp_scores(dist, cases.TASK_COL, dev(unl.astype(np.int32)))
    for strat, row, largest in (("E", "E", True), ("LC", "LC_TASKS", False), ("MS", "MS_TASKS", False)):
        pick = ops.lp_select(sc[O.SCORES[row]], dev(unl.astype(np.int32)), n, 1, largest).item()
        assert unl[pick] == z["%s_pick_%s" % (tag, strat)][0], strat


@pytest.mark.parametrize("tag", cases.LOOP_TAGS)
@pytest.mark.parametrize("strategy", ["E", "LC", "MS"])
def test_query_and_teach_reuse_equals_rebuild_equals_the_oracle_and_scikit_learn(tag, strategy):
    from kgcn_amd import active_learning as al
    z = cases.fixture()
    key, n, d, gamma, alg, variant = cases.parts(tag)
    m = int(z["loop_train"])
    X, truth = z[key + "_X"], z[key + "_truth"]
    picks = {}
    for reuse in (True, False):
        est = al.LabelSpreading(gamma=gamma, alpha=float(z["alpha"])) if alg == "LS" else al.LabelPropagation(gamma=gamma)
        learner = al.ActiveLearner(est, X[:m], truth[:m], query_strategy=strategy)
        picks[reuse] = learner.query_and_teach_n_times(10, X[m:], truth[m:], reuse=reuse)
        assert learner.X_training_vectors.shape == (m + 10, d) and np.array_equal(learner.Y_training[m:], truth[m:][picks[reuse]])
        assert len(learner.n_iter_history_) == 10
    want = O.query_and_teach(X[:m], truth[:m], X[m:], truth[m:], 10, variant, gamma, strategy, float(z["alpha"]), float(z["tol"]))
    assert picks[True] == picks[False] == want == z["%s_loop_%s" % (tag, strategy)].tolist()
