"""The batched C-SVC solver on the GPU (csrc/svm.hip through kgcn_amd/ops.py svm_smo_batch / svm_decision_batch / svm_vote and
kgcn_amd.graph_kernel svm_fit / svm_decision / svm_predict / svm_cv(device=True)): bit for bit against the numpy oracle
(tests/kernel_svm_oracle.py), and within the recorded bound (tests/golden/g15_kernel_svm_bounds.json: ten times the oracle's own
distance) of the decisions scikit-learn recorded in tests/golden/g15_kernel_svm.npz."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import kernel_svm_cases as cases  # noqa: E402
import kernel_svm_oracle as S  # noqa: E402

pytestmark = pytest.mark.gpu

C_EDGES = (1e-4, 2.5, 1e6)          # every alpha at a bound | mixed | no alpha at C


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def gram_dev(name):
    return dev(cases.gram(name))


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def solve(K, problems, tol=1e-3, max_iter=None, iters_per_launch=None):
    """problems [(idx, sign, C)] -> (alpha [P, stride], rho [P], n_iter [P] host arrays, slices, the SvmSets, prob_set)."""
    from kgcn_amd import ops
    uniq, prob_set = [], []
    for idx, sign, _ in problems:                                     # problems that differ only in C share a set
        for s, (i2, s2) in enumerate(uniq):
            if i2 is idx and s2 is sign:
                prob_set.append(s)
                break
        else:
            prob_set.append(len(uniq))
            uniq.append((idx, sign))
    sets = ops.SvmSets([u[0] for u in uniq], [u[1] for u in uniq], graphs=K.shape[0])
    alpha, rho, n_iter, status, slices = ops.svm_smo_batch(K, sets, prob_set, [p[2] for p in problems], tol=tol, max_iter=max_iter,
                                                           iters_per_launch=iters_per_launch)
    assert np.all(status == ops.SVM_CONVERGED)
    return alpha, rho, n_iter, slices, sets, prob_set


def assert_same_as_oracle(Kh, problems, alpha, rho, n_iter, tol=1e-3, max_iter=None):
    a, r, it = alpha.cpu().numpy(), rho.cpu().numpy(), n_iter.cpu().numpy()
    refs = []
    for p, (idx, sign, C) in enumerate(problems):
        ref = S.smo(Kh, idx, sign, C, tol=tol, max_iter=max_iter)
        n = len(idx)
        assert it[p] == ref["n_iter"], (p, n, C, it[p], ref["n_iter"])
        np.testing.assert_array_equal(bits(a[p, :n]), bits(ref["alpha"]), err_msg="alpha of problem %d (n=%d, C=%g)" % (p, n, C))
        assert not a[p, n:].any()
        assert bits(r[p:p + 1])[0] == bits(np.array([ref["rho"]]))[0], (p, n, C, r[p], ref["rho"])
        refs.append(ref)
    return refs


# ---- 1. bits against the oracle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 255, 256, 257, 513, 1024, 1025])
def test_smo_and_decision_bits(n):
    """Every workgroup size and both sides of its thresholds (256 | 257 rows: one wave | four; 1,024 | 1,025: four | sixteen), rows
    permuted, repeated beyond 120 and scattered over K; a plain set and one whose first two entries are the same graph with opposite
    labels (quadratic coefficient 0: TAU); the three C."""
    from kgcn_amd import ops
    name = "sp" if n % 2 else "wl"
    Kh, K = cases.gram(name), gram_dev(name)
    plain, twin = cases.drawn_problem(name, n, n), cases.twin_problem(name, n, n + 1)
    problems = [(i, s, C) for i, s in (plain, twin) for C in C_EDGES]
    alpha, rho, n_iter, _, sets, prob_set = solve(K, problems)
    refs = assert_same_as_oracle(Kh, problems, alpha, rho, n_iter)
    lo, hi = refs[0]["alpha"], refs[2]["alpha"]
    assert np.all((lo == 0.0) | (lo == 1e-4)) and not np.any(hi == 1e6) and np.any(hi > 0.0)
    q = (Kh[twin[0][0], twin[0][0]] + Kh[twin[0][1], twin[0][1]]) - 2.0 * Kh[twin[0][0], twin[0][1]]
    assert q == 0.0 and twin[1][0] != twin[1][1]
    # decisions on every row of K, permuted, and on a short set
    rng = np.random.default_rng(n)
    ev = [rng.permutation(Kh.shape[0]), rng.permutation(Kh.shape[0])[:7]]
    es = ops.SvmSets(ev, graphs=Kh.shape[0])
    jobs = [(p, e) for p in range(len(problems)) for e in range(2)]
    dec, job_out, _ = ops.svm_decision_batch(K, sets, prob_set, alpha, rho, es, [j[0] for j in jobs], [j[1] for j in jobs])
    d = dec.cpu().numpy()
    for q_, (p, e) in enumerate(jobs):
        idx, sign, _ = problems[p]
        want = S.decision(Kh, idx, sign, refs[p]["alpha"], refs[p]["rho"], ev[e])
        np.testing.assert_array_equal(bits(d[job_out[q_]:job_out[q_ + 1]]), bits(want))


# ---- 2. the LDS limit ----------------------------------------------------------------------------------------------------
def test_lds_limit_state_after_max_iter_and_refusal():
    import ctypes
    import torch
    from kgcn_amd import _lib, ops
    Kh = cases.synthetic_gram(4200, 40, 11)
    K = dev(Kh)
    rng = np.random.default_rng(12)
    idx = rng.permutation(4200)[:4096].astype(np.int64)
    sign = np.where(rng.random(4096) < 0.5, 1, -1).astype(np.int8)
    sets = ops.SvmSets([idx], [sign], graphs=4200)
    with pytest.raises(ops.SvmNotConverged) as info:
        ops.svm_smo_batch(K, sets, [0], [2.5], tol=1e-3, max_iter=20)
    assert info.value.problems == [0] and "problem 0 (20 iterations)" in str(info.value)
    alpha, rho, n_iter, status, slices = info.value.result
    assert status.tolist() == [ops.SVM_MAX_ITER] and slices == 1
    ref = assert_same_as_oracle(Kh, [(idx, sign, 2.5)], alpha, rho, n_iter, max_iter=20)[0]
    assert not ref["converged"] and ref["n_iter"] == 20
    # one row more: refused on the host, and by the C entry point, before any launch
    idx2 = rng.permutation(4200)[:4097].astype(np.int64)
    big = ops.SvmSets([idx2], [np.where(np.arange(4097) % 2, 1, -1)], graphs=4200)
    with pytest.raises(_lib.KgcnHipError, match="4097 training rows"):
        ops.svm_smo_batch(K, big, [0], [2.5])
    out = torch.zeros(4097, device="cuda", dtype=torch.float64)
    small = torch.zeros(8, device="cuda", dtype=torch.int64)
    rc = _lib.lib.kgcn_svm_smo_f64(K.data_ptr(), 4200, *big.args(), small.data_ptr(), out.data_ptr(), 1,
                                   ctypes.byref(ctypes.c_double(1e-3)), 0, 16, 1, out.data_ptr(), out.data_ptr(), small.data_ptr(),
                                   small.data_ptr(), out.data_ptr(), 4097 * 8, _lib.current_stream())
    assert rc != 0 and b"4097 training rows" in _lib.lib.kgcn_last_error()
    torch.cuda.synchronize()
    assert not out.any() and not small.any()


# ---- 3. slicing, 4. reproducibility ------------------------------------------------------------------------------------------
def test_slicing_changes_no_bit_and_runs_repeat():
    name = "sp"
    K = gram_dev(name)
    a, b = cases.drawn_problem(name, 257, 21), cases.twin_problem(name, 65, 22)
    problems = [(a[0], a[1], 2.5), (a[0], a[1], 1e-4), (b[0], b[1], 2.5), (b[0], b[1], 1e6)]
    one = solve(K, problems, iters_per_launch=1 << 20)
    cut = solve(K, problems, iters_per_launch=7)
    again = solve(K, problems, iters_per_launch=1 << 20)
    most = int(one[2].max().item())
    assert one[3] == 1 and cut[3] == most // 7 + 1 and most > 7 * 20
    for other in (cut, again):
        for x, y in zip(one[:3], other[:3]):
            assert np.array_equal(x.cpu().numpy().view(np.uint64 if x.dtype.is_floating_point else np.int64),
                                  y.cpu().numpy().view(np.uint64 if y.dtype.is_floating_point else np.int64))
    assert_same_as_oracle(cases.gram(name), problems, *one[:3])


# ---- 5. batch size ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 257])
def test_batch_sizes(P):
    """One problem, and more workgroups than the device has compute units; the problems are 16 (set, C) combinations in turn."""
    name = "wl"
    Kh, K = cases.gram(name), gram_dev(name)
    sets = [cases.drawn_problem(name, n, 30 + n) for n in (50, 77, 96, 120)]
    combos = [(i, s, C) for i, s in sets for C in (1e-4, 2.5, 7.5, 10.0)]
    problems = [combos[(5 * p) % 16] for p in range(P)]
    alpha, rho, n_iter, _, _, prob_set = solve(K, problems)
    assert max(prob_set) == min(P, 4) - 1
    a, r, it = alpha.cpu().numpy(), rho.cpu().numpy(), n_iter.cpu().numpy()
    refs = {}
    for p, (idx, sign, C) in enumerate(problems):
        key = (5 * p) % 16
        if key not in refs:
            refs[key] = S.smo(Kh, idx, sign, C)
        ref, n = refs[key], len(idx)
        assert it[p] == ref["n_iter"] and np.array_equal(bits(a[p, :n]), bits(ref["alpha"])) and bits(r[p:p + 1])[0] == bits(
            np.array([ref["rho"]]))[0], p


# ---- 6. against the fixture, 7. three classes ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fitted(name, lab):
    from kgcn_amd import graph_kernel as gk
    z = cases.fixture()
    folds = cases.folds()
    batch = gk.svm_fit(gram_dev(name), z[lab], [f[0] for f in folds], z["C_grid"], tol=float(z["tol"]))
    evals = [[f[1], f[2]] for f in folds]
    dec = gk.svm_decision(batch, gram_dev(name), evals)
    pred, correct = gk.svm_predict(batch, gram_dev(name), evals, return_correct=True)
    return batch, dec, pred, correct


@pytest.mark.parametrize("lab", ["y2", "y3"])
@pytest.mark.parametrize("name", ["wl", "sp"])
def test_decisions_and_predictions_against_scikit_learn(name, lab):
    """Every row of every fit within the recorded bound; predictions and per-fit accuracies equal on the rows whose reference
    decision is above it; those left out are at most 2 % of the Gram's rows."""
    z = cases.fixture()
    ref_dec, ref_pred, ref_acc = cases.reference(name, lab)
    batch, dec, pred, correct = fitted(name, lab)
    bound = cases.gpu_bound_per_c(name)
    y = z[lab]
    left = total = 0
    worst = 0.0
    for f, c, e in np.ndindex(ref_dec.shape):
        rows = cases.folds()[f][1 + e]
        got, want = dec[f][c][e], ref_dec[f, c, e]
        assert got.shape == want.shape
        worst = max(worst, float(np.abs(got - want).max()))
        assert np.all(np.abs(got - want) <= bound[c]), (f, c, e, float(np.abs(got - want).max()), bound[c])
        keep = np.abs(want).reshape(len(rows), -1).min(axis=1) > bound[c]
        assert np.array_equal(pred[f][c][e][keep], ref_pred[f, c, e][keep]), (f, c, e)
        assert correct[f][c][e] == int((pred[f][c][e] == y[rows]).sum())
        out = int((~keep).sum())
        if out == 0:
            assert correct[f][c][e] / len(rows) == ref_acc[f, c, e]
        else:
            assert abs(correct[f][c][e] - round(ref_acc[f, c, e] * len(rows))) <= out
        left, total = left + out, total + len(rows)
    print("%s %s: largest distance %.3e (bound %.3e), %d of %d rows left out" % (name, lab, worst, bound.max(), left, total))
    assert total == 5400 and left <= cases.LEFT_OUT_CAP * total


# ---- 8. end to end ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lab", ["y2", "y3"])
@pytest.mark.parametrize("name", ["wl", "sp"])
def test_svm_cv_device_route(name, lab):
    from kgcn_amd import graph_kernel as gk
    z = cases.fixture()
    K = gram_dev(name) if lab == "y2" else cases.gram(name)                  # a device tensor or an array
    got = gk.svm_cv(K, z[lab], device=True, tol=float(z["tol"]))
    assert sorted(got) == ["best_C", "fit_indices", "mean", "std", "test_acc", "val_acc"]
    assert all(np.array_equal(a, f[0]) for a, f in zip(got["fit_indices"], cases.folds())) and len(got["fit_indices"]) == 25
    ref_dec = cases.reference(name, lab)[0]
    bound = cases.gpu_bound_per_c(name)
    clean = []
    for o in range(5):                                                  # an outer split none of whose rows was left out
        clean.append(all(np.abs(ref_dec[f, c, e]).min() > bound[c] for f in range(5 * o, 5 * o + 5) for c in range(5) for e in range(2)))
        if clean[-1]:
            for k in ("best_C", "val_acc", "test_acc"):
                assert got[k][o] == z["%s_%s_cv_%s" % (name, lab, k)][o], (k, o)
    if all(clean):
        assert got["mean"] == z["%s_%s_cv_mean" % (name, lab)] and got["std"] == z["%s_%s_cv_std" % (name, lab)]
    print("%s %s: %d of 5 outer splits compared exactly" % (name, lab, sum(clean)))


def test_svm_cv_host_route_is_untouched():
    from kgcn_amd import graph_kernel as gk
    z = cases.fixture()
    got = gk.svm_cv(cases.gram("sp"), z["y2"], tol=float(z["tol"]))
    for k in ("best_C", "val_acc", "test_acc", "mean", "std"):
        assert np.array_equal(np.asarray(got[k], np.float64), z["sp_y2_cv_" + k]), k


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------
def test_one_class_training_set_raises():
    from kgcn_amd import graph_kernel as gk
    y = cases.fixture()["y2"]
    with pytest.raises(ValueError, match="number of classes has to be greater than one"):
        gk.svm_fit(gram_dev("wl"), y, [np.arange(0, 40), np.arange(0, 40, 2)], [1.0])
    with pytest.raises(ValueError):
        gk.svm_cv(gram_dev("wl"), np.zeros(120, np.int64), device=True)


def test_vote_ties_and_bad_descriptors():
    """Three classes, a row whose three pairs tie and a decision of exactly 0; and a job that names a problem out of range."""
    import torch
    from kgcn_amd import _lib, ops
    dec_h = np.array([[1.0, -1.0, 0.0], [-1.0, 1.0, 0.0], [1.0, -1.0, 0.0]])       # pairs x rows, as tests/test_kernel_svm_oracle.py
    ev = ops.SvmSets([[5, 3, 9]], graphs=12)
    labels = torch.zeros(12, dtype=torch.int32, device="cuda")
    labels[9] = 2
    pred, vote_out, counts = ops.svm_vote(dev(dec_h.reshape(-1)), [0, 3, 6, 9], ev, [0], [0], 3, labels)
    assert pred.cpu().tolist() == S.vote(dec_h, 3).tolist() == [0, 0, 2] and counts.cpu().tolist() == [3, 0]
    K = gram_dev("wl")
    idx, sign = cases.drawn_problem("wl", 10, 1)
    alpha, rho, _, _, sets, prob_set = solve(K, [(idx, sign, 1.0)])
    with pytest.raises(ValueError, match="job_prob"):
        ops.svm_decision_batch(K, sets, prob_set, alpha, rho, ev, [1], [0])
    assert isinstance(_lib.KgcnHipError("x"), RuntimeError)
