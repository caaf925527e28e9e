"""The numpy oracle of the batched C-SVC solver (tests/kernel_svm_oracle.py) on its own: the optimality conditions of what it
returns, its distance from the decisions scikit-learn recorded in tests/golden/g15_kernel_svm.npz (the measurement the GPU bound
is ten times of, tests/golden/g15_kernel_svm_bounds.json), and the new entry points and limits of the C header.  No GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import kernel_svm_cases as cases  # noqa: E402
import kernel_svm_oracle as S  # noqa: E402

# |sum y alpha|: every update keeps y_i a_i + y_j a_j up to two roundings of values <= C (C 2^-52 in the worst case, of either
# sign: a drift of about sqrt(iterations) C 2^-53), and the sum of n terms <= C checked here rounds by up to n C 2^-53.  The factor 8
# covers both for the problems below, whose iteration counts stay under (8 n)^2.
SUM_FACTOR = 8.0


@pytest.mark.parametrize("name", ["wl", "sp"])
@pytest.mark.parametrize("n,C,tol", [(2, 2.5, 1e-3), (3, 1e-4, 1e-3), (65, 2.5, 1e-3), (77, 10.0, 1e-10), (120, 1e6, 1e-6),
                                     (257, 2.5, 1e-3)])
def test_oracle_solution_is_feasible_and_optimal(name, n, C, tol):
    K = cases.gram(name)
    idx, sign = cases.twin_problem(name, n, 7) if n == 65 else cases.drawn_problem(name, n, 7)
    r = S.smo(K, idx, sign, C, tol=tol)
    a, y = r["alpha"], sign.astype(np.float64)
    assert r["converged"] and r["n_iter"] < (8 * n) ** 2
    assert np.all(a >= 0.0) and np.all(a <= C)
    assert abs(float(np.sum(y * a))) <= SUM_FACTOR * n * C * 2.0 ** -52
    # m(alpha) - M(alpha) < tol on the gradient the solver carries AND on the one recomputed from alpha
    Q = (y[:, None] * y[None, :]) * K[np.ix_(idx, idx)]
    for G in (r["G"], Q @ a - 1.0):
        up = np.where(y > 0, a < C, a > 0)
        low = np.where(y > 0, a > 0, a < C)
        m = np.max(np.where(up, -y * G, -np.inf))
        M = np.min(np.where(low, -y * G, np.inf))
        slack = 0.0 if G is r["G"] else 1e-9 * max(1.0, C)               # the recomputed gradient rounds differently
        assert m - M < tol + slack, (m - M, tol)


def test_oracle_all_bounded_and_all_free():
    """C = 1e-4 leaves every alpha at its bound (rho: the midpoint), C = 1e6 leaves every support vector free (rho: the mean)."""
    K = cases.gram("wl")
    idx, sign = cases.drawn_problem("wl", 64, 3)
    lo, hi = S.smo(K, idx, sign, 1e-4), S.smo(K, idx, sign, 1e6)
    assert np.all((lo["alpha"] == 0.0) | (lo["alpha"] == 1e-4))
    assert np.all(hi["alpha"] < 1e6) and np.any(hi["alpha"] > 0.0)


def test_oracle_max_iter_returns_the_state_after_that_many_updates():
    K = cases.gram("sp")
    idx, sign = cases.drawn_problem("sp", 100, 5)
    full, cut = S.smo(K, idx, sign, 2.5, tol=1e-10), S.smo(K, idx, sign, 2.5, tol=1e-10, max_iter=20)
    assert full["converged"] and full["n_iter"] > 20
    assert not cut["converged"] and cut["n_iter"] == 20 and np.count_nonzero(cut["alpha"]) <= 40


def test_vote_ties_go_to_the_lowest_class():
    dec = np.array([[1.0, -1.0, 0.0], [-1.0, 1.0, 0.0], [1.0, -1.0, 0.0]])     # pairs (0,1), (0,2), (1,2) x three rows
    # row 0: 0 beats 1, 2 beats 0, 1 beats 2: a three-way tie -> 0.  row 2: dec == 0 votes for the SECOND class of each pair
    assert S.vote(dec, 3).tolist() == [0, 0, 2]
    assert S.vote(np.array([[0.5, 0.0, -0.5]]), 2).tolist() == [0, 1, 1]


@pytest.mark.parametrize("name", ["wl", "sp"])
def test_oracle_distance_from_scikit_learn_is_the_recorded_one(name):
    """All 125 two-class fits and the 25 x 3 three-class problems of the first outer split at tol = 1e-10: no decision is further
    from scikit-learn's than the distance recorded over ALL fits, per C, and the recorded distance is of the order the difference
    between libsvm's float32 kernel rows and fp64 ones explains (1.3e-7 / 4.4e-6 on the first outer split when the issue was
    written)."""
    rec = cases.bounds()[name]
    overall, per_c = cases.distances(name, fits=(None, 5))
    assert np.all(per_c <= np.asarray(rec["distance_per_C"])), (per_c, rec["distance_per_C"])
    assert overall <= rec["distance"] and rec["distance"] == max(rec["distance_per_C"])
    assert 1e-9 < rec["distance"] < 1e-4
    for lab in ("y2", "y3"):                                                # the cap the GPU tests apply, on the reference alone
        n, total = cases.left_out(name, lab, cases.gpu_bound_per_c(name))
        assert total == 5400 and n <= cases.LEFT_OUT_CAP * total, (lab, n, total)


def test_oracle_predictions_equal_the_recorded_ones_off_the_boundary():
    name, lab = "sp", "y3"
    ref, pred, _ = cases.reference(name, lab)
    got, bound = cases.oracle_decisions(name, lab, 5), cases.gpu_bound_per_c(name)
    for f, c, e in np.ndindex(got.shape):
        keep = np.abs(ref[f, c, e]).min(axis=1) > bound[c]
        assert np.array_equal(S.vote(got[f, c, e].T, 3)[keep], pred[f, c, e][keep])


def test_header_declares_the_svm_entry_points_and_limits():
    from kgcn_amd import _lib, ops
    with open(_lib.HEADER_PATH) as f:
        functions, structs, constants = _lib.parse_header(f.read())
    for name in ("kgcn_svm_workspace_bytes", "kgcn_svm_smo_f64", "kgcn_svm_decision_f64", "kgcn_svm_vote_i32"):
        assert name in functions and hasattr(_lib.lib, name)
    assert "kgcn_svm_sets" not in structs                                   # index sets travel as plain arguments
    assert constants["KGCN_HIP_ABI_VERSION"] == 2
    assert ops.SVM_MAX_ROWS == constants["KGCN_SVM_MAX_ROWS"] == 4096
    assert ops.SVM_MAX_CLASSES == constants["KGCN_SVM_MAX_CLASSES"]
    assert ops.SVM_DEFAULT_SLICE == constants["KGCN_SVM_DEFAULT_SLICE"]
    assert (ops.SVM_RUNNING, ops.SVM_CONVERGED, ops.SVM_MAX_ITER, ops.SVM_REFUSED) == (0, 1, 2, 3)
    # G, alpha, QD, the indices and the signs of the longest problem, and the reduction slots, fit the 160 KiB of a CU's LDS
    assert ops.SVM_MAX_ROWS * (3 * 8 + 4 + 1) + 2 * 64 * 8 <= 160 * 1024
    assert _lib.lib.kgcn_svm_workspace_bytes(1, ops.SVM_MAX_ROWS + 1) == -1
    assert b"4096" in _lib.lib.kgcn_last_error() or b"4,096" in _lib.lib.kgcn_last_error()


def test_svm_cv_host_route_is_the_default_and_takes_tol():
    from kgcn_amd import graph_kernel as gk
    z = cases.fixture()
    assert gk.SVM_DEVICE is False
    got = gk.svm_cv(cases.gram("wl"), z["y3"], tol=float(z["tol"]))
    for k in ("best_C", "val_acc", "test_acc", "mean", "std"):
        assert np.array_equal(np.asarray(got[k], np.float64), z["wl_y3_cv_" + k]), k
