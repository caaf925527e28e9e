"""The fixture of the active-learning tests (tests/golden/g16_active_learning.npz, written by tools/gen_active_learning_golden.py with
scikit-learn 1.7.2 and scipy on the host) and what the CPU and the GPU tests both compute from it, once."""
import functools
import json
import os

import numpy as np

import active_learning_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
SETS = ((65, 3), (257, 8), (1025, 32))
GAMMAS = ("g1d", "g20")
ALGS = ("LP", "LS")
TAGS = ["n%d_%s_%s" % (n, g, a) for n, _ in SETS for g in GAMMAS for a in ALGS]
LOOP_TAGS = ["n257_g1d_%s" % a for a in ALGS]
TASK_COL = np.array([0, 2, 5, 7])            # two, three and two classes
TWO_CLASS_COLS, TWO_CLASS_TASK_COL = np.array([0, 1, 5, 6]), np.array([0, 2, 4])


@functools.lru_cache(None)
def fixture():
    with np.load(os.path.join(HERE, "golden", "g16_active_learning.npz")) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(None)
def bounds():
    with open(os.path.join(HERE, "golden", "g16_active_learning_bounds.json")) as f:
        return json.load(f)


def parts(tag):
    key, gname, alg = tag.split("_")
    n = int(key[1:])
    d = dict(SETS)[n]
    return key, n, d, (1.0 / d if gname == "g1d" else 20.0), alg, (O.SPREADING if alg == "LS" else O.PROPAGATION)


def unlabeled(key):
    return np.flatnonzero((fixture()[key + "_Y"] == -1).all(axis=1))


@functools.lru_cache(None)
def oracle_fit(tag):
    """The oracle's (dist, n_iter, classes) on the set of `tag`, from its own affinity matrix."""
    z = fixture()
    key, n, d, gamma, alg, variant = parts(tag)
    W = O.rbf_affinity(z[key + "_X"], gamma)
    dist, n_iter, classes, task_col = O.fit_tasks(W, z[key + "_Y"], variant, float(z["alpha"]), float(z["tol"]), int(z["max_iter"]))
    assert np.array_equal(task_col, TASK_COL)
    dist.setflags(write=False)
    return dist, n_iter, classes
