#!/usr/bin/env python3
"""Generate tests/golden/g12_vecmodal.npz by IMPORTING the reference's numpy half in place (same TensorFlow stub as make_golden.py;
nothing of the reference is copied, only the arrays its functions return) and by asking scikit-learn / numpy for the regression
metrics (scikit-learn 1.7.2 when the committed file was made; the tests read the file, never scikit-learn).

  ds_*     a synthetic stand-in dataset (no dragon / profeat data ships): 120 graphs of 4-12 nodes (rings with self loops and
           two chords), 6 features, `profeat` 70 wide and `dragon` 37 wide (deliberately no multiples of 4), two-class one-hot
           labels and two regression targets that are planted functions of vector and graph, about 15 % of mask_label zero
  info_*   vector_modal_name / vector_modal_dim of the reference's build_data (kgcn/data_util.py:449-455, 558-559)
  feed_*   what construct_feed (kgcn/feed.py:138-157, 201-218) emits for a full batch (graphs 0..49) and a short batch (graphs
           100..119 in a batch of 50): the profeat and dragon feeds, mask, mask_label, enabled_node_nums, and the labels under
           task "regression" (float32) and "classification" (int32)
  r{j}_*   prediction / label sets (float32, as they come off the network) with r2_score, mean_squared_error (gcn.py:205-206) and
           exp(mean(log(label / pred))) (gcn.py:208) on their fp64 values; r{j}_mask, where present, selects the rows scored

    python tests/golden/make_golden_vecmodal.py
"""
import contextlib
import io
import os
import warnings

import numpy as np

from make_golden import HERE, _import_reference

B = 50
FULL, SHORT = list(range(0, 50)), list(range(100, 120))


def dataset(rng):
    G, N, F = 120, 12, 6
    sizes = rng.integers(4, N + 1, G)
    sizes[0], sizes[1] = 4, N
    adj = np.zeros((G, N, N), np.int8)
    feat = np.zeros((G, N, F), np.float32)
    for g, m in enumerate(sizes):
        for i in range(m):
            adj[g, i, i] = adj[g, i, (i + 1) % m] = adj[g, (i + 1) % m, i] = 1
        for _ in range(2):
            i, j = rng.integers(0, m, 2)
            adj[g, i, j] = adj[g, j, i] = 1
        feat[g, :m] = rng.standard_normal((m, F))
    profeat = rng.standard_normal((G, 70)).astype(np.float32)
    dragon = rng.standard_normal((G, 37)).astype(np.float32)
    gmean = np.array([feat[g, :m].mean(axis=0) for g, m in enumerate(sizes)], np.float64)          # [G, F]
    # the class is planted in the vector AND the graph: either alone leaves a third of the graphs wrong
    score = profeat[:, :6].astype(np.float64).mean(axis=1) * 2.0 + gmean[:, 0] * 1.5
    cls = (score > 0).astype(np.int64)
    label_cls = np.stack([1 - cls, cls], axis=1).astype(np.int64)
    d = dragon.astype(np.float64)
    t0 = 2.0 + 0.6 * np.tanh(d[:, :4].sum(axis=1)) + 0.5 * np.tanh(2.0 * gmean[:, 1])
    t1 = 1.5 + 0.4 * d[:, 4] - 0.3 * d[:, 5] + 0.4 * np.tanh(2.0 * gmean[:, 2])
    label_reg = np.stack([t0, t1], axis=1).astype(np.float32)
    mask = (rng.random((G, 2)) >= 0.15).astype(np.float32)
    mask[0] = 0.0
    mask[1] = 1.0
    return dict(dense_adj=adj, feature=feat, sizes=sizes.astype(np.int64), max_node_num=np.int64(N), profeat=profeat, dragon=dragon,
                label_cls=label_cls, label_reg=label_reg, mask_label=mask)


def reference_dict(ds, label):
    """The .jbl dict of docs/dataset_file.md for the stand-in: dense_adj as one [n, n] matrix per graph."""
    return {"feature": ds["feature"], "dense_adj": [ds["dense_adj"][g, :m, :m].astype(np.float32) for g, m in enumerate(ds["sizes"])],
            "max_node_num": int(ds["max_node_num"]), "label": label, "mask_label": ds["mask_label"], "profeat": ds["profeat"],
            "dragon": ds["dragon"]}


def metric_cases(rng):
    cases = []
    y = rng.standard_normal(50) + 2.0
    cases.append(("generic", y, y + 0.3 * rng.standard_normal(50), None))
    cases.append(("constant_target_perfect", np.full(20, 1.25), np.full(20, 1.25), None))
    cases.append(("constant_target_off", np.full(20, 1.25), 1.25 + 0.1 * rng.standard_normal(20), None))
    cases.append(("single_row", np.array([0.75]), np.array([0.5]), None))
    y = rng.random(30) + 0.5
    p = y + 0.1 * rng.standard_normal(30)
    p[7] = -0.25
    cases.append(("negative_ratio", y, p, None))
    y = rng.standard_normal(64) * 2.0 + 5.0
    cases.append(("masked_subset", y, y * (1.0 + 0.1 * rng.standard_normal(64)), (rng.random(64) < 0.6).astype(np.float32)))
    y = rng.random(1000) * 3.0 + 0.1
    cases.append(("thousand_rows", y, y * np.exp(0.2 * rng.standard_normal(1000)), None))
    return [(name, np.asarray(y, np.float32), np.asarray(p, np.float32), m) for name, y, p, m in cases]


def metrics(y, p):
    """gcn.py:205-208 for one task."""
    from sklearn.metrics import mean_squared_error, r2_score
    y, p = y.astype(np.float64), p.astype(np.float64)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        return np.array([r2_score(y, p), mean_squared_error(y, p), np.exp(np.mean(np.log(y / p)))], np.float64)


def main():
    data_util, feed = _import_reference()
    ds = dataset(np.random.default_rng(21))
    out = {"ds_" + k: v for k, v in ds.items()}
    cfg = {"with_feature": True, "with_node_embedding": False, "normalize_adj_flag": False, "split_adj_flag": False, "order": 1,
           "shuffle_data": False}
    placeholders = {k: k for k in ("profeat", "dragon", "labels", "mask", "mask_label", "enabled_node_nums")}
    for task, label in (("regression", ds["label_reg"]), ("classification", ds["label_cls"])):
        c = dict(cfg, task=task)
        with contextlib.redirect_stdout(io.StringIO()):
            all_data, info = data_util.build_data(c, reference_dict(ds, label), prohibit_shuffle=True)
        for tag, idx in (("full", FULL), ("short", SHORT)):
            fd = feed.construct_feed(idx, placeholders, all_data, batch_size=B, info=info, config=c)
            out["feed_%s_labels_%s" % (tag, task)] = fd["labels"]
            if task == "regression":
                for k in ("profeat", "dragon", "mask", "mask_label", "enabled_node_nums"):
                    out["feed_%s_%s" % (tag, k)] = fd[k]
                out["feed_%s_idx" % tag] = np.asarray(idx, np.int64)
    out["feed_batch_size"] = np.int64(B)
    names = sorted(info.vector_modal_name, key=info.vector_modal_name.get)
    out["info_vector_modal_names"] = np.array(names)
    out["info_vector_modal_pos"] = np.array([info.vector_modal_name[n] for n in names], np.int64)
    out["info_vector_modal_dim"] = np.asarray(info.vector_modal_dim, np.int64)
    out["info_label_dim"] = np.int64(info.label_dim)
    cases = metric_cases(np.random.default_rng(22))
    for j, (name, y, p, m) in enumerate(cases):
        out["r%d_label" % j], out["r%d_pred" % j] = y, p
        if m is not None:
            out["r%d_mask" % j] = m
        sel = slice(None) if m is None else m != 0
        out["r%d_metrics" % j] = metrics(y[sel], p[sel])
    out["r_names"] = np.array([c[0] for c in cases])
    out["r_keys"] = np.array(["r2", "mse", "gmfe"])
    import sklearn
    out["sklearn_version"] = np.array(sklearn.__version__)
    np.savez_compressed(os.path.join(HERE, "g12_vecmodal.npz"), **out)
    print("wrote g12_vecmodal.npz: %d graphs, %d metric cases" % (ds["label_cls"].shape[0], len(cases)))
    for j, c in enumerate(cases):
        print("  %-26s" % c[0], out["r%d_metrics" % j])


if __name__ == "__main__":
    main()
