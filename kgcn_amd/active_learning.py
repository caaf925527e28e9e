"""Active learning on the device: the reference's active_learning/models.py (query_next_data_points, ActiveLearner) over the
kernels of csrc/labelprop.hip.

The reference fits scikit-learn's LabelPropagation / LabelSpreading once per task and, in query_and_teach_n_times, again from
scratch for every point it moves from the pool to the training set.  Here one RBF affinity matrix serves all tasks of a query
(fit_tasks), and in the loop one standardised point set and one matrix serve all iterations: a taught row only changes side,
which is a change of the label matrix on the device.  What remains per iteration is the propagation itself (re-initialised, no
warm start: an iteration equals a refit), the scores of the rows still in the pool and the pick, with one word read back per
ops.LP_DEFAULT_CHECK steps.

The affinity matrix need not be stored.  An estimator's attribute matrix_free (set after construction, like max_bytes; False by
default) chooses: False keeps W [n, n] on the device and refuses above max_bytes; True never forms it -- degrees and every step
rebuild its 64 x 64 tiles from the points where they are consumed (ops.rbf_degrees, ops.lp_propagate_free), in O(n (d + classes))
memory and with the stored route's bits; "auto" stores W when it fits max_bytes and goes matrix-free otherwise.  After fit the
estimators predict as scikit-learn's do: predict_proba(X) = rbf_kernel(X, X_) . label_distributions_, normalised by rows, through
ops.rbf_apply (the [m, n] kernel is never formed), predict and score on top of it; after fit_tasks, predict_proba_tasks serves
every task from one such product.

Deviations from the reference, all of them where its own result is unspecified or differs in the last bit only:
  * ties: picks follow a STABLE ascending sort with NaN last (include/kgcn_hip.h, kgcn_lp_select_f64); numpy's default argsort,
    which the reference calls, is not stable, so where scores tie exactly its order is an accident of the sort;
  * "RS" draws from numpy.random.default_rng(seed), not from the global generator;
  * in the reuse route the scaler's sums run over the union [training; pool] in one fixed order, where the reference re-stacks
    the rows every iteration; and the class columns of a task are the classes of the whole loop (a class nobody has been
    taught yet is an all-zero column, which changes no distribution and no score);
  * the variants' scalings (W / s_i; W0 / sqrt(d_i d_j)) are applied to W F instead of being stored in a second matrix.
Refused, not emulated: kernel="knn" and callable kernels, algorithm="SVM" / SVC estimators (Platt scaling with its internal
cross-validation), lists of RDKit molecules (2-D arrays only).  n_jobs is accepted and ignored.
"""
import warnings

import numpy as np
import torch

from . import ops
from ._lib import KgcnHipError

__all__ = ["LabelPropagation", "LabelSpreading", "ConvergenceWarning", "NotFittedError", "query_next_data_points", "ActiveLearner"]


class ConvergenceWarning(UserWarning):
    """A task reached max_iter before sum |F' - F| < tol; n_iter_ = max_iter and the state is returned, as scikit-learn does."""


class NotFittedError(ValueError, AttributeError):
    """predict_proba, predict or score before fit (scikit-learn's exception of the same name has the same two bases)."""


def _check_matrix_free(value):
    if not any(value is v for v in (False, True)) and value != "auto":
        raise ValueError("matrix_free must be False, True or 'auto', got %r" % (value,))
    return value


def _check_kernel(kernel):
    if callable(kernel):
        raise NotImplementedError("callable kernels are not supported: the affinity matrix is built on the device (kernel='rbf')")
    if kernel != "rbf":
        raise NotImplementedError("kernel=%r is not supported, only 'rbf' (the k-nearest-neighbour graph is not built here)" % (kernel,))


def _points(X, name):
    """-> a contiguous [n, d] float64 device tensor; anything but a 2-D array of numbers is refused (no RDKit here)."""
    if isinstance(X, torch.Tensor):
        t = X
    else:
        try:
            a = np.asarray(X, dtype=np.float64)
        except (TypeError, ValueError):
            a = None
        if a is None or a.ndim != 2:
            raise ValueError("%s should be a 2d array of numbers (lists of rdkit.Chem.Mol's are not supported: compute the "
                             "fingerprints first)" % name)
        t = torch.from_numpy(np.ascontiguousarray(a))
    if t.dim() != 2:
        raise ValueError("%s should be a 2d array" % name)
    return t.to(device="cuda", dtype=torch.float64).contiguous()


def encode_labels(Y, classes=None):
    """Y [n, T], -1 = unlabelled -> (labels [n, T] int32: the index of the label among the task's sorted classes or -1; the classes
    of each task; task_col [T + 1]).  classes: take these instead of the ones present in Y."""
    Y = np.asarray(Y)
    if Y.ndim != 2:
        raise ValueError("the labels must be [n, tasks]")
    labels, found, task_col = np.full(Y.shape, -1, np.int32), [], [0]
    for t in range(Y.shape[1]):
        cl = np.unique(Y[:, t]) if classes is None else np.asarray(classes[t])
        cl = cl[cl != -1]
        if cl.shape[0] < 1:
            raise ValueError("task %d has no labelled row" % t)
        for c, v in enumerate(cl):
            labels[Y[:, t] == v, t] = c
        found.append(cl)
        task_col.append(task_col[-1] + cl.shape[0])
    if Y.shape[1] > ops.LP_MAX_TASKS or task_col[-1] > ops.LP_MAX_COLS:
        raise KgcnHipError("%d tasks with %d classes in all; up to %d tasks and %d class columns" % (Y.shape[1], task_col[-1],
                                                                                                 ops.LP_MAX_TASKS, ops.LP_MAX_COLS))
    return labels, found, np.asarray(task_col, np.int64)


class _Graph:
    """One point set on the device, shared by every task and every query over these points: the two degree vectors and either W
    (the stored form) or the points and gamma that W is rebuilt from tile by tile (the matrix-free form, W = None)."""

    def __init__(self, X, gamma, max_bytes=None, matrix_free=False):
        max_bytes = ops.LP_DEFAULT_MAX_BYTES if max_bytes is None else int(max_bytes)
        self.n, self.X, self.gamma = int(X.shape[0]), X, gamma
        if _check_matrix_free(matrix_free) == "auto":
            matrix_free = self.n * self.n * 8 > max_bytes
        if matrix_free:
            self.W = None
            self.s, self.d = ops.rbf_degrees(X, gamma)
        else:
            self.W = ops.rbf_affinity(X, gamma, max_bytes)
            self.s, self.d = ops.lp_degrees(self.W)


class _BaseLabelPropagation:
    _variant = None

    def __init__(self, kernel="rbf", gamma=20, n_neighbors=7, max_iter=1000, tol=1e-3, n_jobs=None):
        self.kernel, self.gamma, self.n_neighbors, self.max_iter, self.tol, self.n_jobs = kernel, gamma, n_neighbors, max_iter, tol, n_jobs
        self.alpha = None
        self.iters_per_check = None
        self.max_bytes = None
        self._matrix_free = False

    @property
    def matrix_free(self):
        """False: store W (refused above max_bytes); True: never store it; "auto": store it when it fits max_bytes."""
        return self._matrix_free

    @matrix_free.setter
    def matrix_free(self, value):
        self._matrix_free = _check_matrix_free(value)

    def get_params(self, deep=True):
        p = {"kernel": self.kernel, "gamma": self.gamma, "n_neighbors": self.n_neighbors, "max_iter": self.max_iter, "tol": self.tol,
             "n_jobs": self.n_jobs}
        if self._variant == ops.LP_SPREADING:
            p["alpha"] = self.alpha
        return p

    # -- the device part: all tasks over one graph
    def _propagate(self, graph, labels_dev, task_col):
        """-> (dist [n, K] device, n_iter [T] device, status [T] device)."""
        _check_kernel(self.kernel)
        spreading = self._variant == ops.LP_SPREADING
        kw = dict(alpha=self.alpha if spreading else 0.2, tol=self.tol, max_iter=self.max_iter, iters_per_check=self.iters_per_check)
        scale = graph.d if spreading else graph.s
        if graph.W is None:
            dist, n_iter, status, _ = ops.lp_propagate_free(graph.X, graph.gamma, scale, labels_dev, task_col, self._variant, **kw)
        else:
            dist, n_iter, status, _ = ops.lp_propagate(graph.W, scale, labels_dev, task_col, self._variant, **kw)
        return dist, n_iter, status

    def _warn(self, status):
        late = np.flatnonzero(np.asarray(status).reshape(-1) == ops.LP_MAX_ITER)
        if late.size:
            warnings.warn("max_iter=%d was reached without convergence (%d task fits)." % (self.max_iter, late.size),
                          category=ConvergenceWarning, stacklevel=3)

    def fit_tasks(self, X, Y):
        """All columns of Y [n, T] (-1 = unlabelled) over ONE affinity matrix of X [n, d].  Sets, as lists over the tasks,
        label_distributions_, transduction_, classes_ and the array n_iter_ [T]."""
        _check_kernel(self.kernel)
        Xd = _points(X, "X")
        labels, classes, task_col = encode_labels(Y)
        if labels.shape[0] != Xd.shape[0]:
            raise ValueError("X has %d rows, Y %d" % (Xd.shape[0], labels.shape[0]))
        graph = _Graph(Xd, self.gamma, self.max_bytes, self.matrix_free)
        dist, n_iter, status = self._propagate(graph, torch.from_numpy(labels).to(Xd.device), task_col)
        self._set(dist.cpu().numpy(), n_iter.cpu().numpy(), status.cpu().numpy(), classes, task_col)
        self.X_, self._dist, self._task_col, self._single = Xd, dist, task_col, False
        self.matrix_free_ = graph.W is None                           # the route this fit took
        return self

    def _set(self, dist, n_iter, status, classes, task_col):
        self._warn(status)
        self.label_distributions_ = [dist[:, task_col[t]:task_col[t + 1]].copy() for t in range(len(classes))]
        self.classes_ = list(classes)
        self.transduction_ = [cl[np.argmax(p, axis=1)] for cl, p in zip(classes, self.label_distributions_)]
        self.n_iter_ = np.asarray(n_iter, np.int64).copy()
        self.status_ = np.asarray(status).copy()

    def fit(self, X, y):
        """scikit-learn's fit: y [n] with -1 = unlabelled; sets label_distributions_ [n, classes], transduction_ [n], classes_ (sorted)
        and n_iter_."""
        y = np.asarray(y)
        if y.ndim != 1:
            raise ValueError("y must be one-dimensional; fit_tasks takes [n, tasks]")
        self.fit_tasks(X, y[:, None])
        self.label_distributions_, self.classes_ = self.label_distributions_[0], self.classes_[0]
        self.transduction_, self.n_iter_ = self.transduction_[0], int(self.n_iter_[0])
        self._single = True
        return self

    # -- prediction: rbf_kernel(X, X_) . label_distributions_ by ops.rbf_apply, on either route
    def _proba(self, X, single):
        if getattr(self, "_dist", None) is None or (single and not self._single):
            raise NotFittedError("this %s instance is not fitted yet: call %s first" % (type(self).__name__,
                                                                                        "fit" if single else "fit or fit_tasks"))
        Xq = _points(X, "X")
        if Xq.shape[1] != self.X_.shape[1]:
            raise ValueError("X has %d attributes, the fitted points %d" % (Xq.shape[1], self.X_.shape[1]))
        raw = ops.rbf_apply(Xq, self.X_, self.gamma, self._dist).cpu().numpy()
        out = []
        with np.errstate(divide="ignore", invalid="ignore"):
            for t in range(len(self._task_col) - 1):                # scikit-learn's division: no guard, a zero row becomes NaN
                block = raw[:, self._task_col[t]:self._task_col[t + 1]]
                norm = np.zeros(block.shape[0])
                for c in range(block.shape[1]):
                    norm = norm + block[:, c]
                out.append(block / norm[:, None])
        return out

    def predict_proba_tasks(self, X):
        """After fit_tasks (or fit): the list over the tasks of [m, classes of the task] probabilities of the rows of X, all tasks
        from ONE product with the kernel between X and the fitted points."""
        return self._proba(X, False)

    def predict_proba(self, X):
        """After fit: [m, classes], rbf_kernel(X, X_) . label_distributions_ with its rows divided by their sums (the task's columns
        added in order from +0.0).  As in scikit-learn a row whose whole kernel row underflows to 0 is NaN."""
        return self._proba(X, True)[0]

    def predict(self, X):
        """classes_[argmax predict_proba(X)]; a NaN row gives classes_[0], as numpy's argmax does in scikit-learn."""
        best = np.argmax(self.predict_proba(X), axis=1)
        return self.classes_[best]

    def score(self, X, y):
        """The mean accuracy of predict(X) against y."""
        return float(np.mean(self.predict(X) == np.asarray(y)))


class LabelPropagation(_BaseLabelPropagation):
    """sklearn.semi_supervised.LabelPropagation with the RBF kernel, on the device."""
    _variant = ops.LP_PROPAGATION


class LabelSpreading(_BaseLabelPropagation):
    """sklearn.semi_supervised.LabelSpreading with the RBF kernel, on the device."""
    _variant = ops.LP_SPREADING

    def __init__(self, kernel="rbf", gamma=20, n_neighbors=7, alpha=0.2, max_iter=1000, tol=1e-3, n_jobs=None):
        super().__init__(kernel, gamma, n_neighbors, max_iter, tol, n_jobs)
        self.alpha = alpha


def _estimator_from(algorithm, kernel, gamma, n_neighbors, max_iter, tol, n_jobs, alpha):
    if algorithm == "SVM":
        raise NotImplementedError("algorithm='SVM' is not supported: SVC(probability=True) is Platt scaling over an internal "
                                  "cross-validation, which is not built here")
    if algorithm == "LP":
        return LabelPropagation(kernel, gamma, n_neighbors, max_iter, tol, n_jobs)
    if algorithm == "LS":
        return LabelSpreading(kernel, gamma, n_neighbors, alpha, max_iter, tol, n_jobs)
    raise ValueError("algorithm must be 'LP' or 'LS', got %r" % (algorithm,))


def unlabeled_rows(Y, label_presence=None):
    """models.py:54-67: (_Y [n, T], the indices of the unlabelled rows).  Without label_presence a row is unlabelled when ALL its
    tasks are -1; with it, the rows it marks False, whose labels are then all set to -1."""
    _Y = np.array(Y, copy=True)
    if _Y.ndim == 1:
        _Y = _Y[:, None]
    if label_presence is None:
        unlabeled = np.flatnonzero((_Y == -1).all(axis=1))
    else:
        unlabeled = np.flatnonzero(np.logical_not(np.asarray(label_presence)))
        _Y[unlabeled] = -1
    return _Y, unlabeled


_QUERY_SCORES = {"E": ("E", True), "LC": ("LC_MEAN", True), "MS": ("MS_MEAN", False)}
_LEARNER_SCORES = {"E": ("E", True), "LC": ("LC_TASKS", False), "MS": ("MS_TASKS", False)}


def query_next_data_points(X, Y, label_presence=None, algorithm="LP", kernel="rbf", gamma=20, n_neighbors=7, max_iter=1000,
                           tol=1e-3, n_jobs=None, alpha=0.2, US_strategy="E", seed=None, matrix_free=False):
    """Up to five indices into X of the unlabelled rows the classifier is least certain about, in the reference's order
    (models.py:18-165): "E" the entropy summed over tasks and "LC" one minus the largest mean probability (the last five of the
    ascending order), "MS" the margin of the mean distribution (its first five), "RS" five random unlabelled rows.
    matrix_free: False, True or "auto", as the estimators' attribute."""
    _check_matrix_free(matrix_free)
    _Y, unlabeled = unlabeled_rows(Y, label_presence)
    if US_strategy == "RS":
        return np.random.default_rng(seed).permutation(unlabeled)[:5]
    if US_strategy not in _QUERY_SCORES:
        raise ValueError("US_strategy must be one of 'E', 'LC', 'MS', 'RS', got %r" % (US_strategy,))
    model = _estimator_from(algorithm, kernel, gamma, n_neighbors, max_iter, tol, n_jobs, alpha)
    _check_kernel(kernel)
    labels, classes, task_col = encode_labels(_Y)
    widths = np.diff(task_col)
    if US_strategy != "E" and (np.any(widths != widths[0]) or (US_strategy == "MS" and widths[0] < 2)):
        raise ValueError("US_strategy=%r averages the tasks' distributions: every task needs the same number of classes%s, got %s"
                         % (US_strategy, " (at least two)" if US_strategy == "MS" else "", widths.tolist()))
    if unlabeled.size == 0:
        return unlabeled
    Xd = _points(X, "X")
    if Xd.shape[0] != labels.shape[0]:
        raise ValueError("X has %d rows, Y %d" % (Xd.shape[0], labels.shape[0]))
    graph = _Graph(Xd, gamma, matrix_free=matrix_free)
    dist, _, status = model._propagate(graph, torch.from_numpy(labels).to(Xd.device), task_col)
    cand = torch.from_numpy(unlabeled.astype(np.int32)).to(Xd.device)
    row, largest = _QUERY_SCORES[US_strategy]
    scores = ops.lp_scores(dist, task_col, cand)
    out = ops.lp_select(scores[ops.LP_SCORES[row]], cand, graph.n, 5, largest).cpu().numpy()
    model._warn(status.cpu().numpy())
    return unlabeled[out[out >= 0]]


class ActiveLearner:
    """models.py:168-343 for 2-D arrays.  estimator: a LabelPropagation / LabelSpreading of this module, or scikit-learn's (recognised
    by class name and read through get_params(); scikit-learn is not imported).  query_strategy: 'E', 'LC', 'MS' or 'RS'."""

    def __init__(self, estimator, X_training, Y_training, finger_print_fn=None, query_strategy="E", seed=None):
        if finger_print_fn is not None:
            raise NotImplementedError("finger_print_fn maps rdkit molecules to vectors; there is no RDKit here: pass 2-D arrays")
        self.estimator = self._adopt(estimator)
        self.X_training_vectors = self._array(X_training, "X_training")
        self.Y_training = np.array(Y_training)
        if self.Y_training.ndim != 2 or self.Y_training.shape[0] != self.X_training_vectors.shape[0]:
            raise ValueError("Y_training should be [len(X_training), tasks]")
        if query_strategy not in ("E", "LC", "MS", "RS"):
            raise ValueError("query_strategy must be one of 'E', 'LC', 'MS', 'RS', got %r" % (query_strategy,))
        self.query_strategy = query_strategy
        self._rng = np.random.default_rng(seed)
        self.n_iter_history_ = []

    @staticmethod
    def _adopt(estimator):
        if isinstance(estimator, _BaseLabelPropagation):
            _check_kernel(estimator.kernel)
            return estimator
        name = type(estimator).__name__
        if name in ("LabelPropagation", "LabelSpreading") and hasattr(estimator, "get_params"):
            p = estimator.get_params()
            _check_kernel(p.get("kernel", "rbf"))
            common = dict(kernel=p.get("kernel", "rbf"), gamma=p.get("gamma", 20), n_neighbors=p.get("n_neighbors", 7),
                          max_iter=p.get("max_iter", 1000), tol=p.get("tol", 1e-3), n_jobs=p.get("n_jobs"))
            return LabelPropagation(**common) if name == "LabelPropagation" else LabelSpreading(alpha=p.get("alpha", 0.2), **common)
        if name in ("SVC", "NuSVC"):
            raise NotImplementedError("SVC estimators are not supported: predict_proba is Platt scaling over an internal "
                                      "cross-validation, which is not built here")
        raise TypeError("estimator must be a LabelPropagation or LabelSpreading (of kgcn_amd.active_learning or scikit-learn), got %s"
                        % name)

    @staticmethod
    def _array(X, name):
        try:
            a = np.asarray(X, dtype=np.float64)
        except (TypeError, ValueError):
            a = None
        if a is None or a.ndim != 2:
            raise ValueError("%s should be a 2d array (lists of rdkit.Chem.Mol's are not supported: compute the fingerprints first)"
                             % name)
        return a

    def _graph(self, X):
        """The standardised points and their graph.  The standardisation is ops.attr_scale: StandardScaler's population-variance
        scaling with a stated summation order, a constant column becoming 0."""
        Xd = _points(X, "X")
        return _Graph(ops.attr_scale(Xd)[0], self.estimator.gamma, self.estimator.max_bytes, self.estimator.matrix_free)

    def query(self, X_pool):
        """-> (the index into X_pool of the row to label next, that row)."""
        pool = self._array(X_pool, "X_pool")
        if self.query_strategy == "RS":
            idx = int(self._rng.integers(len(pool)))
            return idx, X_pool[idx]
        n_train = self.X_training_vectors.shape[0]
        graph = self._graph(np.vstack([self.X_training_vectors, pool]))
        Y = np.vstack([self.Y_training, np.full((len(pool), self.Y_training.shape[1]), -1, self.Y_training.dtype)])
        labels, _, task_col = encode_labels(Y)
        dev = graph.X.device
        dist, n_iter, status = self.estimator._propagate(graph, torch.from_numpy(labels).to(dev), task_col)
        cand = torch.arange(n_train, graph.n, device=dev, dtype=torch.int32)
        row, largest = _LEARNER_SCORES[self.query_strategy]
        scores = ops.lp_scores(dist, task_col, cand)
        idx = int(ops.lp_select(scores[ops.LP_SCORES[row]], cand, graph.n, 1, largest).item())
        self.n_iter_history_.append(n_iter.cpu().numpy())
        self.estimator._warn(status.cpu().numpy())
        return idx, X_pool[idx]

    def teach(self, x_new, y_new):
        self.X_training_vectors = np.vstack([self.X_training_vectors, np.asarray(x_new, np.float64)])
        self.Y_training = np.vstack([self.Y_training, y_new])

    def query_and_teach_n_times(self, n, X_pool, Y_pool, reuse=True):
        """Query and teach n times (-1: the whole pool) -> the ORIGINAL indices into X_pool of the taught rows, in order.
        reuse=True builds the standardised union [training; pool] and its graph once and moves rows on the device; reuse=False
        rebuilds everything per iteration in the reference's row order."""
        pool = self._array(X_pool, "X_pool")
        Y_pool = np.array(Y_pool)
        if Y_pool.ndim != 2 or Y_pool.shape != (len(pool), self.Y_training.shape[1]):
            raise ValueError("Y_pool should be [len(X_pool), tasks]")
        n = len(pool) if n == -1 else int(n)
        if not 0 <= n <= len(pool):
            raise ValueError("%d queries of a pool of %d" % (n, len(pool)))
        if not reuse or self.query_strategy == "RS":
            picked, ind_list = [], list(range(len(pool)))
            for _ in range(n):
                idx, _ = self.query(pool)
                self.teach(pool[idx], Y_pool[idx])
                pool = np.vstack([pool[:idx], pool[idx + 1:]])
                Y_pool = np.vstack([Y_pool[:idx], Y_pool[idx + 1:]])
                picked.append(ind_list.pop(idx))
            return picked
        if n == 0:
            return []
        n_train = self.X_training_vectors.shape[0]
        graph = self._graph(np.vstack([self.X_training_vectors, pool]))
        dev = graph.X.device
        truth = np.vstack([self.Y_training, Y_pool])
        truth_idx, classes, task_col = encode_labels(truth)             # the class columns of the whole loop
        start = truth_idx.copy()
        start[n_train:] = -1
        if np.any((start >= 0).sum(axis=0) == 0):
            raise ValueError("a task has no labelled training row")
        labels, truth_dev = torch.from_numpy(start).to(dev), torch.from_numpy(truth_idx).to(dev)
        active = torch.zeros(graph.n, device=dev, dtype=torch.int32)
        active[n_train:] = 1
        cand = torch.arange(n_train, graph.n, device=dev, dtype=torch.int32)
        picks = torch.full((n,), -1, device=dev, dtype=torch.int32)
        row, largest = _LEARNER_SCORES[self.query_strategy]
        meta = []
        for it in range(n):
            dist, n_iter, status = self.estimator._propagate(graph, labels, task_col)
            scores = ops.lp_scores(dist, task_col, cand)
            ops.lp_select(scores[ops.LP_SCORES[row]], cand, graph.n, 1, largest, active=active, labels=labels, truth=truth_dev,
                          log=picks[it:it + 1])
            meta.append(torch.stack([n_iter, status]))
        picked = [int(p) for p in picks.cpu().numpy()]
        meta = torch.stack(meta).cpu().numpy()
        self.n_iter_history_.extend(meta[:, 0])
        self.estimator._warn(meta[:, 1])
        self.X_training_vectors = np.vstack([self.X_training_vectors, pool[picked]])
        self.Y_training = np.vstack([self.Y_training, Y_pool[picked]])
        return picked
