"""The host side of matrix-free label propagation and of predict_proba (no GPU): the ABI, the estimators' new attribute and
methods before any fit, and the numpy restatement of scikit-learn's predict_proba against tests/golden/g17_lp_predict.npz (written
by tools/gen_lp_predict_golden.py with scikit-learn 1.7.2)."""
import importlib.util
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import active_learning_cases as cases  # noqa: E402
import matrix_free_oracle as MO  # noqa: E402

PREDICT_CASES, case_parts, predict_fixture = MO.PREDICT_CASES, MO.case_parts, MO.predict_fixture


def test_header_declares_the_matrix_free_entry_points():
    from kgcn_amd import _lib
    with open(_lib.HEADER_PATH) as f:
        functions, _, constants = _lib.parse_header(f.read())
    for name in ("kgcn_rbf_apply_f64", "kgcn_rbf_degrees_f64", "kgcn_lp_propagate_free_f64"):
        assert name in functions and hasattr(_lib.lib, name)
    assert constants["KGCN_HIP_ABI_VERSION"] == 2
    stored, free = functions["kgcn_lp_propagate_f64"][1], functions["kgcn_lp_propagate_free_f64"][1]
    assert list(free[-17:]) == list(stored[-17:])                 # one protocol from `scale` on


def test_matrix_free_is_an_attribute_not_a_parameter():
    from kgcn_amd import active_learning as al
    for est in (al.LabelPropagation(), al.LabelSpreading()):
        assert est.matrix_free is False and "matrix_free" not in est.get_params()
        for value in (True, "auto", False):
            est.matrix_free = value
            assert est.matrix_free is value or est.matrix_free == value
        for bad in ("on", 1, 0, None, "AUTO"):
            with pytest.raises(ValueError, match="matrix_free"):
                est.matrix_free = bad
        assert est.matrix_free is False
    with pytest.raises(ValueError, match="matrix_free"):
        al.query_next_data_points(np.zeros((4, 2)), np.array([[0], [1], [-1], [-1]]), matrix_free="yes")


def test_prediction_before_fit_raises():
    from kgcn_amd import active_learning as al
    X = np.zeros((3, 2))
    for est in (al.LabelPropagation(), al.LabelSpreading()):
        for call in (lambda: est.predict_proba(X), lambda: est.predict(X), lambda: est.score(X, np.zeros(3)),
                     lambda: est.predict_proba_tasks(X)):
            with pytest.raises(al.NotFittedError, match="not fitted"):
                call()
    assert issubclass(al.NotFittedError, ValueError) and issubclass(al.NotFittedError, AttributeError)


@pytest.mark.parametrize("case", PREDICT_CASES)
def test_numpy_restatement_of_predict_proba_agrees_with_scikit_learn(case):
    """scikit-learn's own label distributions (recorded in g16) through the restated kernel and division: within 1e-13 of the
    recorded predict_proba (4e-15 was the largest difference measured when the fixture was written), NaN rows in the same places."""
    z, p = cases.fixture(), predict_fixture()
    tag, key, gamma, alg, col = case_parts(case)
    c0, c1 = cases.TASK_COL[col], cases.TASK_COL[col + 1]
    got = MO.predict_proba(z[key + "_X"], z[tag + "_dist"][:, c0:c1], p[key + "_Xq"], gamma)
    want = p[case + "_proba"]
    assert got.shape == want.shape == (33, c1 - c0)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want[-1]).all() and not np.isnan(want[:-1]).all(axis=1).any()
    assert float(np.nanmax(np.abs(got - want))) <= 1e-13
    classes = z[tag + "_classes"][c0:c1]
    pred = classes[np.argmax(got, axis=1)]
    assert np.array_equal(pred, p[case + "_predict"]) and pred[-1] == classes[0]
    assert float(np.mean(pred == p[key + "_truthq"][:, col])) == float(p[case + "_score"])
    top = np.sort(want[:-1][~np.isnan(want[:-1]).any(axis=1)], axis=1)
    assert c1 - c0 < 2 or float((top[:, -1] - top[:, -2]).min()) > float(p["margin"])


def test_the_generator_regenerates_the_committed_fixture():
    pytest.importorskip("sklearn")
    spec = importlib.util.spec_from_file_location("gen_lp_predict_golden", os.path.join(ROOT, "tools", "gen_lp_predict_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert gen.check() == []
