"""What the kernel-SVM tests share: the fixture of tests/golden/make_golden_kernel_svm.py unpacked, the oracle's solutions of all
its fits (computed once), and the synthetic problems of the bit-for-bit tests.  Test infrastructure only."""
import functools
import json
import os

import numpy as np

import kernel_svm_oracle as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g15_kernel_svm.npz")
G13 = os.path.join(ROOT, "tests", "golden", "g13_graph_kernel.npz")
BOUNDS = os.path.join(ROOT, "tests", "golden", "g15_kernel_svm_bounds.json")
GRAMS = {"wl": "two_wl_node_norm", "sp": "two_sp_node_norm"}
BOUND_FACTOR = 10.0           # the project's convention: a GPU bound is ten times the recorded distance of the fp64 restatement
LEFT_OUT_CAP = 0.02           # rows whose reference decision lies within the bound may be at most 2 % of a Gram's rows


@functools.lru_cache(maxsize=None)
def fixture():
    return np.load(GOLDEN, allow_pickle=False)


@functools.lru_cache(maxsize=None)
def gram(name):
    return np.ascontiguousarray(np.load(G13, allow_pickle=False)[GRAMS[name]], dtype=np.float64)


@functools.lru_cache(maxsize=None)
def folds():
    """[(train, val, test)] of the 25 fits."""
    z = fixture()
    cut = lambda n, f: z[n + "_idx"][z[n + "_ptr"][f]:z[n + "_ptr"][f + 1]]  # noqa: E731
    return tuple((cut("train", f), cut("val", f), cut("test", f)) for f in range(len(z["train_ptr"]) - 1))


def labels(lab):
    return fixture()[lab]


def reference(name, lab):
    """-> (dec [F, C, 2] object array of per-set arrays ([rows] or [rows, pairs]), pred likewise, acc [F, C, 2])."""
    z, F, nC = fixture(), len(folds()), len(fixture()["C_grid"])
    dec, pred = z["%s_%s_dec" % (name, lab)], z["%s_%s_pred" % (name, lab)]
    D, Pn = np.empty((F, nC, 2), object), np.empty((F, nC, 2), object)
    pos = 0
    for f, (_, va, te) in enumerate(folds()):
        for c in range(nC):
            for e, rows in enumerate((va, te)):
                D[f, c, e], Pn[f, c, e] = dec[pos:pos + len(rows)], pred[pos:pos + len(rows)]
                pos += len(rows)
    assert pos == len(dec) == len(pred)
    return D, Pn, z["%s_%s_acc" % (name, lab)]


def grouped(codes, train, a, b):
    """The rows of classes a then b of a training set, as libsvm's svm_train groups them, and their signs."""
    rows = np.concatenate([train[codes[train] == a], train[codes[train] == b]])
    return rows, np.where(codes[rows] == a, 1, -1).astype(np.int8)


@functools.lru_cache(maxsize=None)
def oracle_decisions(name, lab, fits=None):
    """The oracle at the fixture's tolerance on every fit (fits: on the first `fits` only) -> dec [F, C, 2] object array shaped as
    reference()'s."""
    z, K, y = fixture(), gram(name), labels(lab)
    k = int(y.max()) + 1
    F, nC = len(folds()) if fits is None else int(fits), len(z["C_grid"])
    D = np.empty((F, nC, 2), object)
    for f, (tr, va, te) in enumerate(folds()[:F]):
        for c, C in enumerate(z["C_grid"]):
            cols = [[], []]
            for a, b in S.pairs(k):
                rows, sign = grouped(y, tr, a, b)
                r = S.smo(K, rows, sign, C, tol=float(z["tol"]))
                assert r["converged"]
                for e, ev in enumerate((va, te)):
                    cols[e].append(S.decision(K, rows, sign, r["alpha"], r["rho"], ev))
            for e in range(2):
                D[f, c, e] = -cols[e][0] if k == 2 else np.stack(cols[e], axis=1)
    return D


def distances(name, fits=(None, None)):
    """The largest |oracle - scikit-learn| decision over both labellings (fits: over the first fits[0] fits of y2 and fits[1] of y3)
    -> (overall, per C [5])."""
    per_c = np.zeros(len(fixture()["C_grid"]))
    for lab, first in zip(("y2", "y3"), fits):
        ref, got = reference(name, lab)[0], oracle_decisions(name, lab, first)
        for f, c, e in np.ndindex(got.shape):
            per_c[c] = max(per_c[c], float(np.abs(ref[f, c, e] - got[f, c, e]).max()))
    return float(per_c.max()), per_c


def left_out(name, lab, bound_per_c):
    """Rows of the reference whose decision (any pair's) lies within the bound of its C -> (count, rows in all)."""
    ref = reference(name, lab)[0]
    count = total = 0
    for f, c, e in np.ndindex(ref.shape):
        d = np.abs(ref[f, c, e]).reshape(len(ref[f, c, e]), -1)
        count += int((d.min(axis=1) <= bound_per_c[c]).sum())
        total += len(d)
    return count, total


@functools.lru_cache(maxsize=None)
def bounds():
    with open(BOUNDS) as f:
        return json.load(f)


def gpu_bound_per_c(name):
    """The bound the GPU tests hold the device to, per C: BOUND_FACTOR x the recorded distance of the Gram -- of that C alone
    where the Gram's one bound would leave more than LEFT_OUT_CAP of the reference's rows undecided."""
    b = bounds()[name]
    return BOUND_FACTOR * np.asarray(b["distance_per_C"] if b["per_C"] else [b["distance"]] * len(b["distance_per_C"]))


# ---- synthetic problems for the bit-for-bit tests -------------------------------------------------------------------------
def drawn_problem(name, n, seed):
    """n training rows drawn from the fixture Gram: a permutation of its rows, repeated where n > 120 (so the sub-matrix is singular
    and rows come from anywhere in K), labels of g13 -- both classes forced to be present."""
    rng = np.random.default_rng(seed)
    G = gram(name).shape[0]
    idx = np.concatenate([rng.permutation(G) for _ in range(-(-n // G))])[:n].astype(np.int64)
    sign = np.where(labels("y2")[idx] == 0, 1, -1).astype(np.int8)
    if n >= 2 and abs(int(sign.sum())) == n:
        sign[0] = -sign[0]
    return idx, sign


def twin_problem(name, n, seed):
    """drawn_problem whose first two entries are the SAME row with opposite labels: Q_00 + Q_11 - 2 Q_01 is 0, the TAU branch."""
    idx, sign = drawn_problem(name, n, seed)
    idx[1], sign[0], sign[1] = idx[0], 1, -1
    return idx, sign


def synthetic_gram(G, rank, seed):
    """A PSD Gram of G rows with a unit diagonal: normalised X X^T of rank `rank`."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((G, rank))
    K = X @ X.T
    d = np.sqrt(np.diag(K))
    K = K / d[:, None] / d[None, :]
    return np.ascontiguousarray((K + K.T) / 2.0)
