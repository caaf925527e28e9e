"""k-fold cross-validation, `kgcn train_cv` (gcn.py:355-524) on the MI355X path: the fold split of scikit-learn's KFold, the
epoch loop of CoreModel.fit (kgcn/core.py:211-370) with early stopping and the best epoch's parameters restored, pred_and_eval
(kgcn/core.py:372-418) and the per-task metrics of compute_metrics (gcn.py:170-256).

The dataset sits in HBM once (data_util.DeviceGraphDataset, labels and mask_label as added tables); folds and epochs are index
lists.  ONE captured training step (train.GraphedTrainStep over FlatParameters / TFAdam) and ONE captured evaluation step serve
every fold: a new fold re-draws the parameters into the flat buffer and zeroes the Adam moments and the step counter in place.
The loss kernel adds each batch's cost and counts into a device block (ops.multitask_softmax2_ce, accum=), so an epoch is read
back once; the predictions of the test fold stay on the device and ops.binary_metrics turns them into the sums behind AUC, AP
and the confusion metrics with one sort.

Deviations from the reference: KFold only (stratified_kfold is refused); the metrics may be restricted to the rows with
mask_label != 0 (config["metrics_mask"], off by default: gcn.py:212 scores every row); no plots; checkpoints are torch.save of
the flat parameter buffer; every fold draws its initial parameters, hold-out split and epoch permutations from its own seeded
generators (seed + fold number), where the reference uses the process-wide numpy state -- a fold can be re-run alone."""
import json
import os
import time

import numpy as np


# ---- splits ---------------------------------------------------------------------------------------------------------------------
def kfold_indices(n, k, shuffle=True, seed=123, stratified=False):
    """KFold(n_splits=k, shuffle=shuffle, random_state=seed).split of n samples (gcn.py:364) -> [(train_idx, test_idx)] * k:
    the indices are shuffled by RandomState(seed) when asked, cut into contiguous folds (the first n % k one longer); the test
    indices of a fold ascend and its train indices are the ascending complement."""
    if stratified:
        raise NotImplementedError("stratified_kfold is not implemented on this path: KFold only (config['stratified_kfold'] = False)")
    n, k = int(n), int(k)
    if k < 2:
        raise ValueError("k-fold cross-validation needs at least 2 folds, got %d" % k)
    if k > n:
        raise ValueError("cannot cut %d samples into %d folds" % (n, k))
    indices = np.arange(n)
    if shuffle:
        np.random.RandomState(seed).shuffle(indices)
    sizes = np.full(k, n // k, dtype=np.int64)
    sizes[:n % k] += 1
    folds, start = [], 0
    for size in sizes:
        test = np.zeros(n, dtype=bool)
        test[indices[start:start + size]] = True
        folds.append((np.nonzero(~test)[0], np.nonzero(test)[0]))
        start += size
    return folds


def holdout_split(n, rate, rng=np.random):
    """split_data (kgcn/data_util.py:612-618): int(n * rate) validation samples off the end of one shuffled arange(n) ->
    (train positions, validation positions)."""
    valid_num = int(n * rate)
    train_num = n - valid_num
    indices = np.arange(n)
    rng.shuffle(indices)
    return indices[:train_num], indices[train_num:n]


class EarlyStopping:
    """kgcn/core.py:15-32: a validation cost above the previous epoch's counts; `patience` such epochs in a row stop the fit
    (patience <= 0 never stops).  The previous cost is replaced whenever the fit goes on."""

    def __init__(self, patience):
        self.patience = int(patience)
        self.prev_validation_cost = None
        self.validation_count = 0

    def evaluate_validation(self, validation_cost):
        if self.prev_validation_cost is not None and self.prev_validation_cost < validation_cost:
            self.validation_count += 1
            if self.patience > 0 and self.validation_count >= self.patience:
                return True
        else:
            self.validation_count = 0
        self.prev_validation_cost = validation_cost
        return False


# ---- metrics --------------------------------------------------------------------------------------------------------------------
def _div(a, b):
    return float(a) / float(b) if b else 0.0


def metrics_from_counts(counts, ap):
    """One task's dict of compute_metrics (gcn.py:210-229) from a row of ops.binary_metrics (n_used, P, TP, FP, n_nonfinite,
    auc_num2, n_groups, spare) and its ap, in fp64: auc = auc_num2 / (2 P N) (roc_curve + auc; NaN without both classes), ap
    (0 without positives, 1 without negatives), acc, pre / rec / f / sup of precision_recall_fscore_support(average='binary')
    (sup is None), balanced_acc (the mean recall of the classes that occur), mcc, jaccard.  A zero division gives 0, as
    scikit-learn answers (with a warning)."""
    n, P, TP, FP = (int(v) for v in counts[:4])
    N, FN = n - P, P - TP
    TN = N - FP
    el = {"auc": float(int(counts[5])) / (2.0 * P * N) if P and N else float("nan"),
          "acc": _div(TP + TN, n),
          "ap": 0.0 if P == 0 else 1.0 if N == 0 else float(ap)}
    pre, rec = _div(TP, TP + FP), _div(TP, P)
    el["pre"], el["rec"], el["f"], el["sup"] = pre, rec, _div(2.0 * pre * rec, pre + rec), None
    recalls = [_div(c, m) for c, m in ((TN, N), (TP, P)) if m]
    el["balanced_acc"] = float(np.mean(recalls)) if recalls else 0.0
    den = float(TP + FP) * float(TP + FN) * float(TN + FP) * float(TN + FN)
    el["mcc"] = (float(TP) * TN - float(FP) * FN) / float(np.sqrt(den)) if den else 0.0
    el["jaccard"] = _div(TP, TP + FP + FN)
    return el


def regression_metrics_from_sums(sums):
    """One task's dict of compute_metrics under config["task"] == "regression" / "regression_gmfe" (gcn.py:204-208) from a row of
    ops.regression_metrics (n, sum y, ss_tot = sum (y - mean y)^2, ss_res = sum (y - p)^2, sum log(y / p), n_bad_ratio), in fp64:
      r2   sklearn.metrics.r2_score: 1 - ss_res / ss_tot; a constant target (ss_tot = 0) gives 1.0 for a perfect prediction,
           else 0.0 (force_finite); fewer than two rows give NaN
      mse  sklearn.metrics.mean_squared_error: ss_res / n (NaN without rows)
      gmfe exp(mean(log(y / p))); NaN when any ratio is <= 0 or not finite (numpy's log of a negative ratio)."""
    n, _, ss_tot, ss_res, slog, bad = (float(v) for v in sums[:6])
    if n < 2:
        r2 = float("nan")
    elif ss_tot != 0.0:
        r2 = 1.0 - ss_res / ss_tot
    else:
        r2 = 1.0 if ss_res == 0.0 else 0.0
    return {"r2": r2, "mse": ss_res / n if n else float("nan"),
            "gmfe": float(np.exp(slog / n)) if n and not bad else float("nan")}


def save_result_cv(result_cv, path):
    """cv.json of gcn.py:492-500: a list over folds of a list over tasks of the metric dicts (NaN is written as json.dump
    writes it, `sup` as null)."""
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, "w") as fp:
        json.dump(result_cv, fp, indent=4)


def auc_table(result_cv, key="auc"):
    """eval.py of the sample: per task the mean and standard deviation of `key` over the folds -> [(task, mean, std)]."""
    tasks = len(result_cv[0])
    rows = []
    for t in range(tasks):
        v = np.array([fold[t][key] for fold in result_cv], np.float64)
        rows.append((t, float(np.nanmean(v)) if np.isfinite(v).any() else float("nan"),
                     float(np.nanstd(v)) if np.isfinite(v).any() else float("nan")))
    return rows


# ---- the fit --------------------------------------------------------------------------------------------------------------------
DEFAULT_CONFIG = {"batch_size": 50, "learning_rate": 1e-3, "patience": 3, "k-fold_num": 5, "validation_data_rate": 0.2,
                  "epoch": 50, "shuffle_data": True, "stratified_kfold": False, "seed": 0, "metrics_mask": False,
                  "threshold": 0.5, "save_result_cv": None, "save_info_cv": None, "save_model_path": None, "task": "classification"}
TASKS = ("classification", "regression")


class CrossValidator:
    """The captured steps and device state that all folds share.  model_factory() -> a fresh network taking
    (features, adjacency) and returning logits [B, 2, T] (models.CPIMultitaskNet); dataset: data_util.DeviceGraphDataset;
    labels / mask_label: [G, T] arrays.
    forward_tables: {keyword: [G, ...] array or device tensor} of further per-graph inputs of the network (the vector modality,
    data_util.vector_table: {"vectors": table}); each is registered with the static batch and handed to every forward call --
    warm-up, captured training step, captured evaluation step, reset -- under its keyword.
    config["task"] = "regression" (gcn.py:204-206, kgcn/core.py:184-186): the network returns predictions [B, T]
    (models.MultimodalRegressionGCN), the loss is ops.masked_squared_error, the epoch summaries carry mse = error_sum / count in
    place of the accuracy, and a test fold's metric dicts are regression_metrics_from_sums' {"r2", "mse", "gmfe"}."""

    def __init__(self, model_factory, dataset, labels, mask_label, config=None, forward_tables=None):
        import torch
        from . import ops, train
        self.config = dict(DEFAULT_CONFIG)
        self.config.update(config or {})
        unknown = set(self.config) - set(DEFAULT_CONFIG)
        if unknown:
            raise ValueError("unknown train_cv settings: %s" % sorted(unknown))
        kfold_indices(2, 2, stratified=self.config["stratified_kfold"])                 # refuses what is not implemented, early
        if self.config["task"] not in TASKS:
            raise ValueError("config['task'] must be one of %s, got %r" % (TASKS, self.config["task"]))
        self.regression = regression = self.config["task"] == "regression"
        # a dead hipGraph that only the cycle collector can free must go NOW: destroying one while a stream captures is an error
        # that ends the process, and torch.cuda.graph() no longer collects on entry
        import gc
        gc.collect()
        self.factory, self.dataset = model_factory, dataset
        dev = dataset.channels[0].rowptr.device
        self.labels = torch.as_tensor(np.ascontiguousarray(labels, dtype=np.float32), device=dev)
        self.mask_label = torch.as_tensor(np.ascontiguousarray(mask_label, dtype=np.float32), device=dev)
        G = dataset.num_graphs
        if self.labels.dim() != 2 or tuple(self.labels.shape) != tuple(self.mask_label.shape) or self.labels.shape[0] != G:
            raise ValueError("labels and mask_label must be [%d graphs, tasks] arrays" % G)
        self.tasks = T = int(self.labels.shape[1])
        self.batch_size = B = int(self.config["batch_size"])
        self.batch = dataset.static_batch(B)
        self.lab = self.batch.add_table(self.labels)
        self.ml = self.batch.add_table(self.mask_label)
        self.kw = {}
        for name, table in (forward_tables or {}).items():
            t = table if torch.is_tensor(table) else torch.as_tensor(np.ascontiguousarray(table, dtype=np.float32))
            if t.shape[0] != G:
                raise ValueError("forward table %r has %d rows for %d graphs" % (name, t.shape[0], G))
            self.kw[name] = self.batch.add_table(t.to(dev))
        self.batch.load(np.arange(min(B, G)))
        torch.manual_seed(int(self.config["seed"]))
        self.model = model_factory().to(dev)
        self.model(self.batch.features, self.batch.adjacency, **self.kw)                # creates the parameters (lazy build)
        self.opt = train.TFAdam(self.model.parameters(), lr=float(self.config["learning_rate"]))
        self.flat = self.opt.flat
        # [each_cost | each_correct | each_count | cost] of the batches since the last zero_(): training and evaluation
        # (regression: [error_sum | count | cost_sum], ops.masked_squared_error)
        self.train_sums = torch.zeros((2 if regression else 3) * T + 1, device=dev)
        self.eval_sums = torch.zeros_like(self.train_sums)
        self.best = torch.empty_like(self.flat.data)

        sums = self.train_sums                         # not `self`: a closure over self would tie the validator into a reference

        def loss_fn(logits, labels_, mask_):           # cycle, and its hipGraphs would then die whenever the collector runs
            if regression:
                return ops.masked_squared_error(logits, labels_, mask_, accum=sums)[:2]
            cost = ops.multitask_softmax2_ce(logits, labels_, mask_, accum=sums)[0]
            return cost, cost

        self.step = train.GraphedTrainStep(self.model, self.opt, loss_fn, self.batch, self.lab, self.ml, capture_assembly=True,
                                           **self.kw)
        # the evaluation step: assembly, forward and loss (sums into eval_sums, predictions at a fixed address)
        self.prediction = None
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                self._evaluate()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.eval_graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.eval_graph, **train.capture_mode()):
            self._evaluate()
        self.train_sums.zero_()
        self.eval_sums.zero_()

    def _evaluate(self):
        import torch
        from . import ops
        with torch.no_grad():
            ops.weight_tables.refresh()
            self.batch.assemble()
            logits = self.model(self.batch.features, self.batch.adjacency, **self.kw)
            if self.regression:
                ops.masked_squared_error(logits, self.lab, self.ml, accum=self.eval_sums)
                self.prediction = logits
            else:
                self.prediction = ops.multitask_softmax2_ce(logits, self.lab, self.ml, accum=self.eval_sums)[4]

    # -- state of a fold ----------------------------------------------------------------------------------------------------------
    def reset(self, seed):
        """A fresh fit in place: parameters re-drawn by a model_factory() network built under torch.manual_seed(seed), Adam
        moments and step counter zeroed.  The captured steps keep reading the same buffers."""
        import torch
        from . import ops
        torch.manual_seed(int(seed))
        fresh = self.factory().to(self.flat.data.device)
        with torch.no_grad():
            fresh(self.batch.features, self.batch.adjacency, **self.kw)
            new = list(fresh.parameters())
            if [tuple(p.shape) for p in new] != [tuple(p.shape) for p in self.flat.params]:
                raise RuntimeError("model_factory() built a network with other parameters than the captured one")
            torch._foreach_copy_(self.flat.views, [p.data for p in new])
            self.opt._m.zero_()
            self.opt._v.zero_()
            self.opt._t_dev.zero_()
        self.opt.t = 0
        ops.weight_tables.invalidate()                 # the weights changed behind torch's version counters

    def restore(self, flat_values):
        from . import ops
        self.flat.data.copy_(flat_values)
        ops.weight_tables.invalidate()

    def _summary(self, sums, T, num):
        s = sums.double().cpu().numpy()                # the one read-back of an epoch / an evaluation
        if self.regression:
            # kgcn/core.py:184-186: mse = error_sum / count over all tasks (the model's metrics are scalars); per task beside it
            with np.errstate(divide="ignore", invalid="ignore"):
                each_mse = s[:T] / s[T:2 * T]
                mse = float(s[:T].sum() / s[T:2 * T].sum())
            return float(s[2 * T]) / num, mse, each_mse
        with np.errstate(divide="ignore", invalid="ignore"):
            each_acc = s[T:2 * T] / s[2 * T:3 * T]
        # kgcn/core.py:200-206: each_accuracy = each_correct_count / each_count, accuracy = its nanmean
        acc = float(np.nanmean(each_acc)) if np.isfinite(each_acc).any() else float("nan")
        return float(s[3 * T]) / num, acc, each_acc

    def _train_epoch(self, idx):
        B = self.batch_size
        self.train_sums.zero_()
        for it in range(0, len(idx), B):
            self.batch.stage(idx[it:it + B])
            self.step.replay()
        return self._summary(self.train_sums, self.tasks, len(idx))

    def pred_and_eval(self, idx):
        """kgcn/core.py:372-418 over the graphs `idx` -> (cost per graph, accuracy, predictions [len(idx), T] on the device)."""
        import torch
        B, T = self.batch_size, self.tasks
        idx = np.asarray(idx, np.int64)
        pred = torch.empty((len(idx), T), device=self.flat.data.device, dtype=torch.float32)
        self.eval_sums.zero_()
        for it in range(0, len(idx), B):
            nb = min(B, len(idx) - it)
            self.batch.stage(idx[it:it + nb])
            self.eval_graph.replay()
            pred[it:it + nb].copy_(self.prediction[:nb])
        cost, acc, _ = self._summary(self.eval_sums, T, max(len(idx), 1))
        return cost, acc, pred

    def fit(self, train_idx, valid_idx, seed, validation_cost_fn=None, fold=None):
        """CoreModel.fit (kgcn/core.py:211-370) on the graphs train_idx / valid_idx from a fresh state (reset(seed)); the epoch
        permutations come from RandomState(seed).  The parameters of the epoch with the lowest validation cost are kept in a
        device snapshot and restored at the end (:340-356).  validation_cost_fn(epoch, cost) -> cost replaces the validation
        cost that early stopping and the best-epoch choice see (a test hook).  -> dict of the per-epoch lists."""
        cfg = self.config
        self.reset(seed)
        rs = np.random.RandomState(int(seed))
        train_idx = np.array(train_idx, np.int64)
        valid_idx = np.asarray(valid_idx, np.int64)
        stopper = EarlyStopping(cfg["patience"])
        acc = "mse" if self.regression else "acc"
        out = {"training_cost": [], "validation_cost": [], "training_" + acc: [], "validation_" + acc: [], "best_epoch": None}
        best = None
        for epoch in range(int(cfg["epoch"])):
            rs.shuffle(train_idx)                                                      # kgcn/core.py:248
            tcost, tacc, _ = self._train_epoch(train_idx)
            if len(valid_idx):
                vcost, vacc, _ = self.pred_and_eval(valid_idx)
            else:
                vcost, vacc = 0.0, 0.0
            out["training_cost"].append(tcost)
            out["training_" + acc].append(tacc)
            if len(valid_idx):
                out["validation_cost"].append(vcost)
                out["validation_" + acc].append(vacc)
            seen = vcost if validation_cost_fn is None else float(validation_cost_fn(epoch, vcost))
            if stopper.evaluate_validation(seen) or np.isnan(seen):
                break
            if best is None or best > seen:
                best = seen
                out["best_epoch"] = epoch
                self.best.copy_(self.flat.data)
        path = cfg["save_model_path"]
        if path:
            import torch
            os.makedirs(path, exist_ok=True)
            tag = "" if fold is None else "%03d." % fold
            torch.save(self.flat.data.cpu(), os.path.join(path, "model.%slast.pt" % tag))
            if best is not None:
                torch.save(self.best.cpu(), os.path.join(path, "model.%sbest.pt" % tag))
        if best is not None:
            self.restore(self.best)
        return out

    def run_fold(self, fold, train_valid_idx, test_idx, validation_cost_fn=None):
        """One iteration of gcn.py:383-450: hold-out split of the fold's training graphs, fit, the test fold scored with the
        best epoch's parameters -> (metric dicts per task, info dict, predictions [n_test, T] on the device)."""
        import torch
        from . import ops
        cfg = self.config
        seed = int(cfg["seed"]) + int(fold)
        train_valid_idx = np.asarray(train_valid_idx, np.int64)
        test_idx = np.asarray(test_idx, np.int64)
        tr, va = holdout_split(len(train_valid_idx), cfg["validation_data_rate"], np.random.RandomState(seed))
        t0 = time.time()
        info = self.fit(train_valid_idx[tr], train_valid_idx[va], seed, validation_cost_fn, fold=fold)
        torch.cuda.synchronize()
        info["train_time"] = time.time() - t0
        t0 = time.time()
        cost, acc, pred = self.pred_and_eval(test_idx)
        sel = torch.as_tensor(test_idx, device=pred.device)
        mask = self.mask_label.index_select(0, sel) if cfg["metrics_mask"] else None
        if self.regression:
            sums = ops.regression_metrics(pred, self.labels.index_select(0, sel), mask)
            info["infer_time"] = time.time() - t0
            info.update(test_cost=cost, test_mse=acc, test_data_idx=[int(i) for i in test_idx], sums=sums.tolist())
            return [regression_metrics_from_sums(sums[t]) for t in range(self.tasks)], info, pred
        counts, ap = ops.binary_metrics(pred, self.labels.index_select(0, sel), mask, threshold=cfg["threshold"])
        info["infer_time"] = time.time() - t0
        info.update(test_cost=cost, test_acc=acc, test_data_idx=[int(i) for i in test_idx], counts=counts.tolist(), ap=ap.tolist())
        return [metrics_from_counts(counts[t], ap[t]) for t in range(self.tasks)], info, pred

    def run(self, validation_cost_fn=None):
        cfg = self.config
        folds = kfold_indices(self.dataset.num_graphs, cfg["k-fold_num"], cfg["shuffle_data"], stratified=cfg["stratified_kfold"])
        result_cv, info_cv, predictions = [], [], []
        for fold, (train_valid_idx, test_idx) in enumerate(folds, 1):
            v, info, pred = self.run_fold(fold, train_valid_idx, test_idx, validation_cost_fn)
            result_cv.append(v)
            info_cv.append(info)
            predictions.append(pred)
        if cfg["save_result_cv"]:
            save_result_cv(result_cv, cfg["save_result_cv"])
        if cfg["save_info_cv"]:
            save_result_cv(info_cv, cfg["save_info_cv"])
        return {"result_cv": result_cv, "info_cv": info_cv, "predictions": predictions, "folds": folds}


def train_cv(model_factory, dataset, labels, mask_label, config=None, forward_tables=None):
    """gcn.py train_cv -> {"result_cv": cv.json's content, "info_cv": the save_info_cv fields per fold (costs and accuracies
    per epoch, best_epoch, test_cost, test_acc, test_data_idx, train_time, infer_time, the metric sums), "predictions": the
    test folds' [n_test, T] device tensors, "folds": the (train, test) index pairs}.  config: DEFAULT_CONFIG's keys (the names
    of the reference's config where it has them); save_result_cv / save_info_cv write the two JSON files."""
    return CrossValidator(model_factory, dataset, labels, mask_label, config, forward_tables).run()
