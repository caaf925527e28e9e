"""Writes tests/golden/g17_lp_predict.npz: what scikit-learn 1.7.2 gives, on the host, for predict_proba / predict / score of
LabelPropagation and LabelSpreading (RBF kernel) on the point sets n65 and n257 of tests/golden/g16_active_learning.npz.  Run from
the repository root on a machine with scikit-learn:

    python tools/gen_lp_predict_golden.py            # writes the fixture
    python tools/gen_lp_predict_golden.py --check    # regenerates it in memory and compares it with the committed file

Per set: 33 queries -- 20 training points perturbed by 0.05 standard normal, two exact training points, ten standard-normal points
and one far point at 1e3 in every attribute (its kernel row underflows: scikit-learn divides 0 by 0 and returns a NaN row, and
predict gives classes_[0] there) -- and their `truth` [33, 3]: the truth of the source point, for the random and the far point
that of the nearest training point.  Per (set, gamma = 1 / d "g1d" or 20 "g20", LP / LS, label column): predict_proba, predict and
score(queries, truth).  Every row that is not NaN must have its two largest probabilities more than MARGIN apart in every case,
so that predict is unambiguous; otherwise the next query seed is drawn.  The seed used is recorded."""
import os
import sys
import warnings

import numpy as np
from sklearn.exceptions import ConvergenceWarning
from sklearn.semi_supervised import LabelPropagation, LabelSpreading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "golden", "g16_active_learning.npz")
OUT = os.path.join(ROOT, "tests", "golden", "g17_lp_predict.npz")
SETS = ((65, 3), (257, 8))
MARGIN = 1e-3
PERTURBED, EXACT, RANDOM = 20, 2, 10


class Replace(Exception):
    pass


def queries(X, truth, seed):
    rng = np.random.default_rng(seed)
    n, d = X.shape
    src = rng.permutation(n)[:PERTURBED + EXACT]
    Xq = np.vstack([X[src[:PERTURBED]] + 0.05 * rng.standard_normal((PERTURBED, d)), X[src[PERTURBED:]],
                    rng.standard_normal((RANDOM, d)), np.full((1, d), 1e3)])
    nearest = np.argmin(((Xq[PERTURBED + EXACT:, None, :] - X[None, :, :]) ** 2).sum(axis=2), axis=1)
    return Xq, np.vstack([truth[src], truth[nearest]])


def one_set(z, n, d, seed, rec):
    key = "n%d" % n
    X, Y, truth = z[key + "_X"], z[key + "_Y"], z[key + "_truth"]
    Xq, tq = queries(X, truth, seed)
    rec[key + "_Xq"], rec[key + "_truthq"], rec[key + "_qseed"] = Xq, tq, np.int64(seed)
    worst = np.inf
    for gname, gamma in (("g1d", 1.0 / d), ("g20", 20.0)):
        for alg in ("LP", "LS"):
            for col in range(Y.shape[1]):
                kw = dict(kernel="rbf", gamma=gamma, max_iter=int(z["max_iter"]), tol=float(z["tol"]))
                m = LabelPropagation(**kw) if alg == "LP" else LabelSpreading(alpha=float(z["alpha"]), **kw)
                with warnings.catch_warnings(), np.errstate(divide="ignore", invalid="ignore"):
                    warnings.simplefilter("ignore", ConvergenceWarning)
                    warnings.simplefilter("ignore", RuntimeWarning)
                    m.fit(X, Y[:, col])
                    proba = m.predict_proba(Xq)
                    pred = m.predict(Xq)
                    score = m.score(Xq, tq[:, col])
                tag = "%s_%s_%s_c%d" % (key, gname, alg, col)
                nan = np.isnan(proba).any(axis=1)
                if not nan[-1] or nan[:PERTURBED + EXACT].any():
                    raise Replace("%s: NaN rows %s" % (tag, np.flatnonzero(nan)))
                top = np.sort(proba[~nan], axis=1)
                margin = float((top[:, -1] - top[:, -2]).min())
                if not margin > MARGIN:
                    raise Replace("%s: margin %.3g" % (tag, margin))
                worst = min(worst, margin)
                rec[tag + "_proba"], rec[tag + "_predict"], rec[tag + "_score"] = proba, pred, np.float64(score)
    return worst


def generate():
    with np.load(SRC) as f:
        z = {k: f[k] for k in f.files}
    rec = {"margin": np.float64(MARGIN)}
    for n, d in SETS:
        for seed in range(100):
            trial = dict(rec)
            try:
                worst = one_set(z, n, d, seed, trial)
            except Replace as e:
                print("n = %d query seed %d replaced: %s" % (n, seed, e))
                continue
            print("n = %d: query seed %d, smallest margin %.3g" % (n, seed, worst))
            rec = trial
            break
        else:
            raise SystemExit("no query seed below 100 serves the %d-point set" % n)
    return rec


def check():
    """-> the names whose regenerated value differs from the committed file (probabilities by 1e-12, everything else exactly)."""
    rec = generate()
    with np.load(OUT) as f:
        have = {k: f[k] for k in f.files}
    bad = sorted(set(rec) ^ set(have))
    for k in sorted(set(rec) & set(have)):
        a, b = np.asarray(rec[k]), have[k]
        same = a.shape == b.shape and (np.allclose(a, b, rtol=0.0, atol=1e-12, equal_nan=True) if k.endswith("_proba")
                                       else np.array_equal(a, b))
        if not same:
            bad.append(k)
    return bad


def main():
    if "--check" in sys.argv[1:]:
        bad = check()
        print("differs: %s" % bad if bad else "%s is what this machine regenerates" % OUT)
        raise SystemExit(1 if bad else 0)
    rec = generate()
    np.savez_compressed(OUT, **rec)
    print("wrote %s (%d bytes, %d arrays)" % (OUT, os.path.getsize(OUT), len(rec)))


if __name__ == "__main__":
    main()
