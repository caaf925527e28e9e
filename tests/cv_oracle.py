"""numpy fp64 statement of the cross-validation workflow (gcn.py train_cv) for the tests: the network and loss of
sample_chem/compound-protein_interaction/multitask.py from the layer functions of oracle/kgcn_oracle.py, and the binary
metrics of gcn.py:170-256 (compute_metrics) from their definitions -- the sums the device kernel reports (exact integers) and
every metric derived from them.  scikit-learn is not read here: tests/golden/make_golden_cv.py records its answers in
tests/golden/g11_cv.npz and tests/test_cv_host.py holds this file to them."""
import numpy as np

from oracle import kgcn_oracle as K

COLUMNS = ("n_used", "P", "TP", "FP", "n_nonfinite", "auc_num2", "n_groups", "spare")
METRIC_KEYS = ("auc", "acc", "ap", "pre", "rec", "f", "balanced_acc", "mcc", "jaccard")


# ---- metrics -----------------------------------------------------------------------------------------------------------------
def binary_sums(score, label, mask=None, threshold=0.5):
    """One task: score [n] (float32 values), label [n], mask [n] or None -> (the eight integers of COLUMNS as Python ints, ap
    as a float, G the number of distinct scores).  Groups are the distinct scores in descending order (-0.0 == +0.0);
    auc_num2 = sum_g (fp_g - fp_g-1) (tp_g + tp_g-1);  ap = sum_g ((tp_g - tp_g-1) / P) (tp_g / (tp_g + fp_g)), 0 for P = 0."""
    score = np.asarray(score, np.float32).reshape(-1)
    label = np.asarray(label).reshape(-1) != 0
    if mask is not None:
        keep = np.asarray(mask).reshape(-1) != 0
        score, label = score[keep], label[keep]
    n = int(score.shape[0])
    P = int(label.sum())
    above = score > np.float32(threshold)
    TP, FP = int((above & label).sum()), int((above & ~label).sum())
    nonfinite = int((~np.isfinite(score)).sum())
    if nonfinite:
        return [n, P, TP, FP, nonfinite, 0, 0, 0], 0.0, 0
    order = np.argsort(-score.astype(np.float64), kind="stable")
    s, l = score[order], label[order]
    ends = np.r_[np.nonzero(s[1:] != s[:-1])[0], n - 1] if n else np.zeros(0, np.int64)
    tp = np.cumsum(l)[ends].astype(object) if n else np.zeros(0, object)         # Python integers: no overflow
    fp = (ends + 1).astype(object) - tp if n else np.zeros(0, object)
    tp0, fp0 = np.r_[0, tp[:-1]] if n else tp, np.r_[0, fp[:-1]] if n else fp
    auc_num2 = int(sum((fp - fp0) * (tp + tp0))) if n else 0
    ap = 0.0
    if P:
        tpf, fpf, tp0f = tp.astype(np.float64), fp.astype(np.float64), tp0.astype(np.float64)
        for g in range(len(ends)):                                                  # descending threshold, one running sum
            ap += ((tpf[g] - tp0f[g]) / P) * (tpf[g] / (tpf[g] + fpf[g]))
    return [n, P, TP, FP, 0, auc_num2, int(len(ends)), 0], float(ap), int(len(ends))


def binary_sums_all(score, label, mask=None, threshold=0.5):
    """All tasks: score / label / mask [n, T] -> (counts [T, 8] int64, ap [T] float64, G [T])."""
    score = np.asarray(score)
    T = score.shape[1]
    rows = [binary_sums(score[:, t], np.asarray(label)[:, t], None if mask is None else np.asarray(mask)[:, t], threshold)
            for t in range(T)]
    return (np.array([r[0] for r in rows], np.int64).reshape(T, 8), np.array([r[1] for r in rows], np.float64),
            np.array([r[2] for r in rows], np.int64))


def _div(a, b):
    return float(a) / float(b) if b else 0.0


def metrics(counts, ap):
    """The dict of compute_metrics for one task from its sums (fp64; a zero division gives 0 as scikit-learn's
    zero_division='warn' does, AUC is NaN without both classes, AP 0 without positives and 1 without negatives)."""
    n, P, TP, FP = (int(v) for v in counts[:4])
    N, FN = n - P, P - TP
    TN = N - FP
    el = {"auc": float(counts[5]) / (2.0 * P * N) if P and N else float("nan"),
          "acc": _div(TP + TN, n),
          "ap": (0.0 if P == 0 else 1.0 if N == 0 else float(ap))}
    pre, rec = _div(TP, TP + FP), _div(TP, P)
    el["pre"], el["rec"], el["f"], el["sup"] = pre, rec, _div(2.0 * pre * rec, pre + rec), None
    per_class = [_div(c, k) for c, k in ((TN, N), (TP, P)) if k]                    # recall of the classes that occur
    el["balanced_acc"] = float(np.mean(per_class)) if per_class else 0.0
    den = float(TP + FP) * float(TP + FN) * float(TN + FP) * float(TN + FN)
    el["mcc"] = (float(TP) * TN - float(FP) * FN) / np.sqrt(den) if den else 0.0
    el["jaccard"] = _div(TP, TP + FP + FN)
    return el


# ---- the loss head (multitask.py:53-86) -----------------------------------------------------------------------------------------
def softmax2_ce(logits, labels, mask_label):
    """logits [B, 2, T], labels / mask_label [B, T] -> dict(cost, each_cost, each_correct, each_count, prediction, dlogits)."""
    z = np.asarray(logits, np.float64)
    y = np.asarray(labels) != 0
    m = np.asarray(mask_label) != 0
    d = z[:, 1, :] - z[:, 0, :]
    u = np.where(y, -d, d)
    ce = np.maximum(u, 0.0) + np.log1p(np.exp(-np.abs(u)))
    e = np.exp(-np.abs(d))
    p1 = np.where(d >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    g1 = np.where(m, p1 - y, 0.0)
    each_cost = (ce * m).sum(axis=0)
    return {"cost": float(each_cost.sum()), "each_cost": each_cost, "each_correct": (((d > 0) == y) & m).sum(axis=0),
            "each_count": m.sum(axis=0), "prediction": p1, "dlogits": np.stack([-g1, g1], axis=1)}


# ---- the network (multitask.py:35-51) ----------------------------------------------------------------------------------------
def model_fwd(x, adjs, p):
    """GraphConv(512) -> sigmoid -> GraphGather -> Dense(2 T), logits[b, c, t] = out[b, c T + t].  p: w / b (lists over the
    adjacency channels), kernel [512, 2 T], bias [2 T]."""
    pre = K.graphconv_fwd(x, adjs, p["w"], p["b"])
    act = 1.0 / (1.0 + np.exp(-pre))
    pooled = K.gather_fwd(act)
    out = pooled @ np.asarray(p["kernel"], np.float64) + np.asarray(p["bias"], np.float64)
    B = out.shape[0]
    return out.reshape(B, 2, -1), {"act": act, "pooled": pooled}


def model_loss_grads(x, adjs, p, labels, mask_label):
    """-> (loss dict of softmax2_ce, logits, gradients {w: [..], b: [..], kernel, bias} of the cost)."""
    logits, c = model_fwd(x, adjs, p)
    L = softmax2_ce(logits, labels, mask_label)
    B = logits.shape[0]
    dout = L["dlogits"].reshape(B, -1)
    dpooled = dout @ np.asarray(p["kernel"], np.float64).T
    dact = K.gather_bwd(dpooled, c["act"].shape[1])
    dpre = dact * c["act"] * (1.0 - c["act"])
    _, dw, db = K.graphconv_bwd(x, adjs, p["w"], p["b"], dpre)
    return L, logits, {"w": dw, "b": [t.reshape(-1) for t in db], "kernel": c["pooled"].T @ dout, "bias": dout.sum(axis=0)}
