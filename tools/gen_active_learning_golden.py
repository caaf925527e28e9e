"""Writes tests/golden/g16_active_learning.npz and g16_active_learning_bounds.json: what scikit-learn 1.7.2 and scipy give, on the
host, for the point sets the active-learning tests use.  Run from the repository root on a machine with scikit-learn:

    python tools/gen_active_learning_golden.py

Point sets: standardised Gaussian blobs, three clusters, at (n, d) = (65, 3), (257, 8), (1025, 32), each with gamma = 1 / d ("g1d")
and with the reference's default gamma = 20 ("g20").  Label matrix Y [n, 3]: task 0 two classes, task 1 three, task 2 two; about a
fifth of the rows labelled per task, independently, so rows are labelled in one task and -1 in another, and some in none.
Recorded per (set, gamma, algorithm LP / LS, task): label_distributions_, n_iter_, transduction_, classes_ of scikit-learn's
estimator and scipy.stats.entropy of the unlabelled rows.  On the g1d sets only: the five picks of query_next_data_points per
strategy, the single pick of ActiveLearner.query, and on the 257-point set ten rounds of query_and_teach_n_times with
scikit-learn refitted from scratch each round.

The bounds file records TEN TIMES the distance of tests/active_learning_oracle.py from scikit-learn, measured here; its "gpu"
section (what the GPU tests measured against the oracle) is kept as it is found.  A set is REPLACED (the next seed is drawn, and
the seed recorded), never skipped, when
  * a convergence sum next to the decision (the last two checks of a fit) lies within n * classes * bound of tol, or
  * a recorded selection has a score gap, at a rank that is compared, below 1,000 times the score bound.
"""
import json
import os
import sys
import warnings

import numpy as np
from scipy import stats
from sklearn.exceptions import ConvergenceWarning
from sklearn.preprocessing import StandardScaler
from sklearn.semi_supervised import LabelPropagation, LabelSpreading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import active_learning_oracle as O  # noqa: E402

SETS = ((65, 3), (257, 8), (1025, 32))
ALPHA, TOL, MAX_ITER = 0.2, 1e-3, 1000
GAP_FACTOR = 1000.0
LOOP_SET, LOOP_TRAIN, LOOP_ROUNDS = 257, 40, 10
OUT = os.path.join(ROOT, "tests", "golden", "g16_active_learning.npz")
BOUNDS = os.path.join(ROOT, "tests", "golden", "g16_active_learning_bounds.json")


class Replace(Exception):
    pass


def draw(n, d, seed):
    rng = np.random.default_rng(seed)
    centres = 2.5 * rng.standard_normal((3, d))
    cluster = rng.integers(0, 3, n)
    cluster[:3] = (0, 1, 2)
    X = centres[cluster] + rng.standard_normal((n, d))
    X = (X - X.mean(axis=0)) / X.std(axis=0)
    truth = np.stack([(cluster == 0).astype(np.int64), cluster.astype(np.int64) + 3, (cluster == 2).astype(np.int64) * 5], axis=1)
    flip = rng.random((n, 3)) < 0.05                            # some label noise, so that the clusters are not the whole story
    truth = np.where(flip, np.roll(truth, 1, axis=0), truth)
    shown = rng.random((n, 3)) < 0.2
    shown[:6] = True                                            # every class of every task is labelled at least once
    truth[:6] = np.stack([(np.arange(6) % 3 == 0), np.arange(6) % 3 + 3, (np.arange(6) % 3 == 2) * 5], axis=1)
    return X, np.where(shown, truth, -1), truth


def estimator(alg, gamma, max_iter=MAX_ITER):
    if alg == "LP":
        return LabelPropagation(kernel="rbf", gamma=gamma, max_iter=max_iter, tol=TOL)
    return LabelSpreading(kernel="rbf", gamma=gamma, alpha=ALPHA, max_iter=max_iter, tol=TOL)


def fit_all(X, Y, alg, gamma):
    out = []
    for t in range(Y.shape[1]):
        m = estimator(alg, gamma)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", ConvergenceWarning)
            m.fit(X, Y[:, t])
        out.append(m)
    return out


def gaps_ok(score, order, bound, what):
    """order: the positions compared, in ascending score; every adjacent pair, and the neighbour outside, is GAP_FACTOR bounds apart."""
    s = np.sort(score[~np.isnan(score)])
    pos = np.searchsorted(s, np.sort(score[order]))
    lo, hi = max(pos.min() - 1, 0), min(pos.max() + 1, len(s) - 1)
    gap = np.diff(s[lo:hi + 1]).min() if hi > lo else np.inf
    if not gap >= GAP_FACTOR * bound:
        raise Replace("%s: score gap %.3g below %g x %.3g" % (what, gap, GAP_FACTOR, bound))
    return float(gap)


def one_set(n, d, seed, rec, bounds):
    X, Y, truth = draw(n, d, seed)
    key = "n%d" % n
    rec[key + "_X"], rec[key + "_Y"], rec[key + "_truth"], rec[key + "_seed"] = X, Y, truth, np.int64(seed)
    unl = np.flatnonzero((Y == -1).all(axis=1))
    assert unl.size >= 6
    for gname, gamma in (("g1d", 1.0 / d), ("g20", 20.0)):
        W = O.rbf_affinity(X, gamma)
        for alg in ("LP", "LS"):
            variant = O.SPREADING if alg == "LS" else O.PROPAGATION
            models = fit_all(X, Y, alg, gamma)
            labels, classes, task_col = O.encode(Y)
            s, dg = O.degrees(W)
            r = O.propagate(W, dg if variant else s, labels, task_col, variant, ALPHA, TOL, MAX_ITER)
            dist = O.finish(r["F"], task_col)
            sk = np.concatenate([m.label_distributions_ for m in models], axis=1)
            tag = "%s_%s_%s" % (key, gname, alg)
            distance = float(np.abs(dist - sk).max())
            n_iter = np.array([m.n_iter_ for m in models])
            if not np.array_equal(n_iter, r["n_iter"]):
                raise Replace("%s: n_iter %s, the oracle's %s" % (tag, n_iter, r["n_iter"]))
            for t in range(3):                                   # the two convergence sums next to the decision stay clear of tol
                k = int(n_iter[t])
                near = [r["sums"][j][t] for j in (k - 1, k) if 0 <= j < len(r["sums"]) and k < MAX_ITER]
                room = n * (task_col[t + 1] - task_col[t]) * 10.0 * max(distance, 2.0 ** -52)
                if any(abs(v - TOL) <= room for v in near):
                    raise Replace("%s task %d: convergence sum %s within %.3g of tol" % (tag, t, near, room))
            ent = np.stack([stats.entropy(m.label_distributions_[unl].T) for m in models])
            sc_sk, sc_or = O.scores(sk, task_col, unl), O.scores(dist, task_col, unl)
            e_distance = float(np.nanmax(np.abs(sc_or[O.SCORES["E"]] - ent.sum(axis=0))))
            rec[tag + "_dist"], rec[tag + "_n_iter"], rec[tag + "_entropy"] = sk, n_iter, ent
            rec[tag + "_transduction"] = np.stack([m.transduction_ for m in models], axis=1)
            rec[tag + "_classes"] = np.concatenate([m.classes_ for m in models])
            b = {"distance": distance, "bound": 10.0 * distance, "entropy_distance": e_distance, "n_iter": n_iter.tolist()}
            if gname == "g1d":
                # the scores that are ranked: E over the three tasks, LC / MS over the two two-class tasks (0 and 2)
                cols2 = np.r_[task_col[0]:task_col[1], task_col[2]:task_col[3]]
                tc2 = np.array([0, 2, 4])
                s2_sk, s2_or = O.scores(sk[:, cols2], tc2, unl), O.scores(dist[:, cols2], tc2, unl)
                score_distance = float(max(np.nanmax(np.abs(sc_sk - sc_or)), np.nanmax(np.abs(s2_sk - s2_or)), e_distance))
                sb = 10.0 * max(score_distance, bounds.get("gpu", {}).get("score_distance", 0.0))
                b["score_distance"], b["score_bound"], b["gaps"] = score_distance, 10.0 * score_distance, {}
                for strat, src, row, largest in (("E", sc_sk, "E", True), ("LC", s2_sk, "LC_MEAN", True), ("MS", s2_sk, "MS_MEAN", False)):
                    pick = O.select(src[O.SCORES[row]], 5, largest)
                    b["gaps"]["top5_" + strat] = gaps_ok(src[O.SCORES[row]], pick, sb, tag + " top5 " + strat)
                    rec["%s_top5_%s" % (tag, strat)] = unl[pick]
                for strat, row, largest in (("E", "E", True), ("LC", "LC_TASKS", False), ("MS", "MS_TASKS", False)):
                    pick = O.select(sc_sk[O.SCORES[row]], 1, largest)
                    b["gaps"]["pick_" + strat] = gaps_ok(sc_sk[O.SCORES[row]], pick, sb, tag + " pick " + strat)
                    rec["%s_pick_%s" % (tag, strat)] = unl[pick]
                if n == LOOP_SET:
                    for strat in ("E", "LC", "MS"):
                        rec["%s_loop_%s" % (tag, strat)] = loop(X, truth, alg, gamma, strat, sb, tag)
            bounds["fits"][tag] = b


def loop(X, truth, alg, gamma, strat, sb, tag):
    """query_and_teach_n_times with scikit-learn: StandardScaler and one estimator a task refitted from scratch each round, rows
    stacked [training; taught; pool left] as the reference stacks them.  -> the original pool indices."""
    Xt, Yt, Xp, Yp = X[:LOOP_TRAIN], truth[:LOOP_TRAIN], X[LOOP_TRAIN:], truth[LOOP_TRAIN:]
    left, picked = list(range(len(Xp))), []
    row, largest = {"E": ("E", True), "LC": ("LC_TASKS", False), "MS": ("MS_TASKS", False)}[strat]
    for rnd in range(LOOP_ROUNDS):
        Xn = StandardScaler().fit_transform(np.vstack([Xt, Xp]))
        Y = np.vstack([Yt, np.full((len(Xp), 3), -1)])
        models = fit_all(Xn, Y, alg, gamma)
        sk = np.concatenate([m.label_distributions_ for m in models], axis=1)
        task_col = np.concatenate([[0], np.cumsum([len(m.classes_) for m in models])])
        score = O.scores(sk, task_col, np.arange(len(Xt), len(Xn)))[O.SCORES[row]]
        p = O.select(score, 1, largest)
        gaps_ok(score, p, sb, "%s loop %s round %d" % (tag, strat, rnd))
        p = int(p[0])
        Xt, Yt = np.vstack([Xt, Xp[p]]), np.vstack([Yt, Yp[p]])
        Xp, Yp = np.delete(Xp, p, axis=0), np.delete(Yp, p, axis=0)
        picked.append(left.pop(p))
    return np.array(picked)


def main():
    bounds = {"fits": {}, "seeds": {}}
    if os.path.exists(BOUNDS):
        with open(BOUNDS) as f:
            bounds["gpu"] = json.load(f).get("gpu", {})
    rec = {"alpha": np.float64(ALPHA), "tol": np.float64(TOL), "max_iter": np.int64(MAX_ITER), "loop_train": np.int64(LOOP_TRAIN)}
    for n, d in SETS:
        for seed in range(100):
            trial, tb = dict(rec), {"fits": dict(bounds["fits"]), "gpu": bounds.get("gpu", {})}
            try:
                one_set(n, d, seed, trial, tb)
            except Replace as e:
                print("n = %d seed %d replaced: %s" % (n, seed, e))
                continue
            rec, bounds["fits"], bounds["seeds"]["n%d" % n] = trial, tb["fits"], seed
            break
        else:
            raise SystemExit("no seed below 100 gives a usable set of %d points" % n)
    import sklearn
    import scipy
    bounds["versions"] = {"scikit-learn": sklearn.__version__, "scipy": scipy.__version__, "numpy": np.__version__}
    bounds["convention"] = "bound = 10 x distance; distance = max |oracle - scikit-learn| over the label distributions, measured on the host"
    np.savez_compressed(OUT, **rec)
    with open(BOUNDS, "w") as f:
        json.dump(bounds, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s (%d bytes) and %s" % (OUT, os.path.getsize(OUT), BOUNDS))
    for k, v in sorted(bounds["fits"].items()):
        print(k, "distance %.3g" % v["distance"], "n_iter", v["n_iter"], "entropy %.3g" % v["entropy_distance"],
              "score %.3g" % v.get("score_distance", float("nan")))


if __name__ == "__main__":
    main()
