"""The numpy oracle of the active-learning kernels (tests/active_learning_oracle.py) against what scikit-learn and scipy recorded in
tests/golden/g16_active_learning.npz, within tests/golden/g16_active_learning_bounds.json; the host logic of
kgcn_amd/active_learning.py (which rows are unlabelled, label_presence, the index bookkeeping of query_and_teach_n_times, the
refusals); and the new entry points of the C header.  No GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import active_learning_cases as cases  # noqa: E402
import active_learning_oracle as O  # noqa: E402


@pytest.mark.parametrize("tag", cases.TAGS)
def test_oracle_against_scikit_learn_within_the_recorded_bounds(tag):
    z, b = cases.fixture(), cases.bounds()["fits"][tag]
    dist, n_iter, classes = cases.oracle_fit(tag)
    assert b["bound"] == 10.0 * b["distance"] and b["distance"] < 1e-12
    assert float(np.abs(dist - z[tag + "_dist"]).max()) <= b["distance"]
    assert np.array_equal(n_iter, z[tag + "_n_iter"]) and n_iter.tolist() == b["n_iter"]
    assert np.array_equal(np.concatenate(classes), z[tag + "_classes"])
    trans = np.stack([classes[t][np.argmax(dist[:, cases.TASK_COL[t]:cases.TASK_COL[t + 1]], axis=1)] for t in range(3)], axis=1)
    assert np.array_equal(trans, z[tag + "_transduction"])
    key = tag.split("_")[0]
    unl = cases.unlabeled(key)
    E = O.scores(dist, cases.TASK_COL, unl)[O.SCORES["E"]]
    assert float(np.abs(E - z[tag + "_entropy"].sum(axis=0)).max()) <= b["entropy_distance"]


def test_fixture_covers_max_iter_and_long_runs():
    n_iter = {t: cases.bounds()["fits"][t]["n_iter"] for t in cases.TAGS}
    assert any(max(v) == 1000 for v in n_iter.values())          # the reference's gamma = 20 runs LabelPropagation into max_iter
    assert all(max(n_iter["n%d_g1d_LS" % n]) <= 8 for n, _ in cases.SETS)


@pytest.mark.parametrize("tag", [t for t in cases.TAGS if "_g1d_" in t])
def test_oracle_selections_equal_the_recorded_ones(tag):
    z = cases.fixture()
    dist, _, _ = cases.oracle_fit(tag)
    unl = cases.unlabeled(tag.split("_")[0])
    sc = O.scores(dist, cases.TASK_COL, unl)
    sc2 = O.scores(dist[:, cases.TWO_CLASS_COLS], cases.TWO_CLASS_TASK_COL, unl)
    for strat, src, row, largest in (("E", sc, "E", True), ("LC", sc2, "LC_MEAN", True), ("MS", sc2, "MS_MEAN", False)):
        assert np.array_equal(unl[O.select(src[O.SCORES[row]], 5, largest)], z["%s_top5_%s" % (tag, strat)]), strat
    for strat, row, largest in (("E", "E", True), ("LC", "LC_TASKS", False), ("MS", "MS_TASKS", False)):
        assert np.array_equal(unl[O.select(sc[O.SCORES[row]], 1, largest)], z["%s_pick_%s" % (tag, strat)]), strat


@pytest.mark.parametrize("tag", cases.LOOP_TAGS)
@pytest.mark.parametrize("strategy", ["E", "LC", "MS"])
def test_oracle_loop_over_the_fixed_union_picks_what_scikit_learn_refits_pick(tag, strategy):
    z = cases.fixture()
    key, n, d, gamma, alg, variant = cases.parts(tag)
    m = int(z["loop_train"])
    X, truth = z[key + "_X"], z[key + "_truth"]
    got = O.query_and_teach(X[:m], truth[:m], X[m:], truth[m:], 10, variant, gamma, strategy, float(z["alpha"]), float(z["tol"]))
    assert got == z["%s_loop_%s" % (tag, strategy)].tolist()


def test_product_orders_and_degrees():
    rng = np.random.default_rng(0)
    for n in (1, 2, 63, 64, 65, 130):
        W, G = rng.random((n, n)), rng.random((n, 3))
        assert np.allclose(O.product(W, G), W @ G, rtol=1e-13, atol=0)
        s, d = O.degrees(W)
        assert np.allclose(s, W.sum(axis=1), rtol=1e-13) and np.allclose(d, W.sum(axis=1) - np.diag(W), rtol=1e-12, atol=1e-15)
    # the stated order, on a case where the order shows: lane 0 adds 1 + 2^-53 + 2^-53 (lost twice), the tree adds lane 1's 2^-52
    W = np.zeros((1, 130))
    W[0, [0, 64, 128, 1]] = 1.0, 2.0 ** -53, 2.0 ** -53, 2.0 ** -52
    assert O.product(W, np.ones((130, 1)))[0, 0] == 1.0 + 2.0 ** -52


def test_select_is_stable_with_nan_last():
    s = np.array([0.5, np.nan, 0.5, 0.1, 0.5, np.nan, 0.1])
    assert O.select(s, 5, True).tolist() == [0, 2, 4, 1, 5]       # the last five of [3, 6, 0, 2, 4, 1, 5]
    assert O.select(s, 5, False).tolist() == [3, 6, 0, 2, 4]
    assert O.select(s, 1, True).tolist() == [5] and O.select(s, 1, False).tolist() == [3]
    part = np.array([1, 0, 1, 0, 1, 0, 1], bool)
    assert O.select(s, 5, True, part).tolist() == [6, 0, 2, 4] and O.select(s, 1, False, part).tolist() == [6]


def test_scores_of_a_zero_row_and_of_a_one_class_task():
    dist = np.array([[0.25, 0.75, 1.0, 0.5, 0.5], [0.0, 0.0, 1.0, 1.0, 0.0]])
    sc = O.scores(dist, np.array([0, 2, 3, 5]), [0, 1])
    e0 = -(0.25 * np.log(0.25) + 0.75 * np.log(0.75)) + 0.0 + np.log(2.0)
    assert abs(sc[O.SCORES["E"], 0] - e0) < 1e-15 and np.isnan(sc[O.SCORES["E"], 1])
    assert sc[O.SCORES["MS_TASKS"]].tolist() == [0.5 + 1.0 + 0.0, 0.0 + 1.0 + 1.0]     # a one-class task's margin is its column
    assert sc[O.SCORES["LC_TASKS"]].tolist() == [(0.75 + 1.0 + 0.5) / 3, (0.0 + 1.0 + 1.0) / 3]
    assert np.isnan(sc[O.SCORES["LC_MEAN"]]).all()                # the tasks' class counts differ: no mean distribution


# ---- host logic of kgcn_amd/active_learning.py ---------------------------------------------------------------------------------
def test_unlabelled_rule_and_label_presence():
    from kgcn_amd import active_learning as al
    Y = np.array([[0, -1], [-1, -1], [1, 2], [-1, 3], [-1, -1]])
    _Y, unl = al.unlabeled_rows(Y)
    assert unl.tolist() == [1, 4] and np.array_equal(_Y, Y)      # unlabelled: -1 in ALL tasks
    _Y, unl = al.unlabeled_rows(Y, label_presence=[True, True, False, True, False])
    assert unl.tolist() == [2, 4] and _Y[2].tolist() == [-1, -1] and _Y[1].tolist() == [-1, -1] and _Y[0].tolist() == [0, -1]
    assert Y[2].tolist() == [1, 2]                                # the caller's labels are not written
    _Y, unl = al.unlabeled_rows(np.array([0, -1, 1]))
    assert _Y.shape == (3, 1) and unl.tolist() == [1]
    labels, classes, task_col = al.encode_labels(np.array([[5, -1], [3, 7], [-1, 7], [5, 9]]))
    assert labels.tolist() == [[1, -1], [0, 0], [-1, 0], [1, 1]] and task_col.tolist() == [0, 2, 4]
    assert [c.tolist() for c in classes] == [[3, 5], [7, 9]]
    with pytest.raises(ValueError):
        al.encode_labels(np.array([[0, -1], [1, -1]]))


def test_random_strategy_is_seeded_and_keeps_the_books():
    from kgcn_amd import active_learning as al
    Y = np.array([[0], [-1], [1], [-1], [-1], [-1], [-1], [-1]])
    X = np.arange(16.0).reshape(8, 2)
    a = al.query_next_data_points(X, Y, US_strategy="RS", seed=3)
    assert a.tolist() == al.query_next_data_points(X, Y, US_strategy="RS", seed=3).tolist()
    assert len(a) == 5 and set(a) <= {1, 3, 4, 5, 6, 7}
    learner = al.ActiveLearner(al.LabelSpreading(gamma=0.5), X[:2], [[0], [1]], query_strategy="RS", seed=1)
    pool, Ypool = X[2:], np.arange(6)[:, None] % 2
    picked = learner.query_and_teach_n_times(4, pool, Ypool)
    assert len(set(picked)) == 4 and set(picked) <= set(range(6))             # ORIGINAL pool indices, none twice
    assert np.array_equal(learner.X_training_vectors[2:], pool[picked]) and np.array_equal(learner.Y_training[2:], Ypool[picked])
    assert len(al.ActiveLearner(al.LabelSpreading(), X[:2], [[0], [1]], query_strategy="RS", seed=1)
               .query_and_teach_n_times(-1, pool, Ypool)) == 6


def test_refusals_are_errors_not_emulations():
    from kgcn_amd import active_learning as al
    X, Y = np.zeros((4, 2)), np.array([[0], [1], [-1], [-1]])
    with pytest.raises(NotImplementedError, match="knn"):
        al.query_next_data_points(X, Y, kernel="knn")
    with pytest.raises(NotImplementedError, match="callable"):
        al.LabelPropagation(kernel=lambda a, b: a @ b.T).fit_tasks(X, Y)
    with pytest.raises(NotImplementedError, match="SVM"):
        al.query_next_data_points(X, Y, algorithm="SVM")
    with pytest.raises(ValueError, match="same number of classes"):
        al.query_next_data_points(X, np.array([[0, 0], [1, 1], [-1, 2], [-1, -1]]), US_strategy="LC")

    class SVC:
        pass

    class LabelSpreading:                                         # scikit-learn's, as far as ActiveLearner looks: name and get_params
        def get_params(self):
            return {"kernel": "rbf", "gamma": 0.25, "alpha": 0.4, "max_iter": 30, "tol": 1e-4, "n_jobs": 4, "n_neighbors": 7}

    class LabelPropagation(LabelSpreading):
        def get_params(self):
            return {"kernel": "knn"}
    with pytest.raises(NotImplementedError, match="SVC"):
        al.ActiveLearner(SVC(), X[:2], Y[:2])
    with pytest.raises(NotImplementedError, match="knn"):
        al.ActiveLearner(LabelPropagation(), X[:2], Y[:2])
    with pytest.raises(ValueError, match="rdkit"):
        al.ActiveLearner(al.LabelPropagation(), [object(), object()], Y[:2])
    with pytest.raises(TypeError):
        al.ActiveLearner(object(), X[:2], Y[:2])
    est = al.ActiveLearner(LabelSpreading(), X[:2], Y[:2]).estimator
    assert isinstance(est, al.LabelSpreading) and (est.gamma, est.alpha, est.max_iter, est.tol, est.n_jobs) == (0.25, 0.4, 30, 1e-4, 4)


def test_header_declares_the_active_learning_entry_points():
    from kgcn_amd import _lib, ops
    with open(_lib.HEADER_PATH) as f:
        functions, _, constants = _lib.parse_header(f.read())
    for name in ("kgcn_rbf_affinity_f64", "kgcn_lp_degrees_f64", "kgcn_lp_workspace_bytes", "kgcn_lp_propagate_f64",
                 "kgcn_lp_finish_f64", "kgcn_lp_scores_f64", "kgcn_lp_select_f64"):
        assert name in functions and hasattr(_lib.lib, name)
    assert constants["KGCN_HIP_ABI_VERSION"] == 2
    assert ops.LP_BLOCK_ROWS == constants["KGCN_LP_BLOCK_ROWS"] == O.BLOCK_ROWS == 32
    assert (ops.LP_PROPAGATION, ops.LP_SPREADING) == (O.PROPAGATION, O.SPREADING)
    assert (ops.LP_RUNNING, ops.LP_CONVERGED, ops.LP_MAX_ITER) == (O.RUNNING, O.CONVERGED, O.MAX_ITER)
    assert ops.LP_SCORES == O.SCORES
    assert _lib.lib.kgcn_lp_workspace_bytes(10, ops.LP_MAX_TASKS + 1, ops.LP_MAX_COLS) == -1
    assert _lib.lib.kgcn_lp_workspace_bytes(1000, 4, 8) >= 4 * 1000 * 8 * 8 + 32 * 4 * 8
