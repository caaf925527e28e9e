#!/usr/bin/env python3
"""The vector-modality models on the MI355X path:

  --model vec         example_model/model_multimodal_vec.py: GraphConv branch + Dense/BatchNormalization/relu tower 300/100/64 on
                      the per-graph vector `profeat`, shared Dense(52)+BN+relu, Dense(label_dim), softmax cross entropy
  --model regression  example_model/model_multimodal_regression.py: GraphDense/GraphBatchNormalization branch + Dense(8)+BN+relu
                      on `dragon`, Dense(label_dim), masked squared error

Graphs, features, the vector table, labels and masks live in HBM (data_util.DeviceGraphDataset + StaticBatch.add_table); a step is
one small index upload and ONE hipGraph replay (assembly, forward, loss, backward, Adam).  After every epoch: the training cost per
graph and, on a 0.2 validation split (kgcn/data_util.py:612-618), the cost and the accuracy (vec) or mse = error_sum / count
(regression, kgcn/core.py:184-186).

No dragon / profeat dataset ships, so the default is the synthetic stand-in of tests/golden/g12_vecmodal.npz (120 graphs of
4-12 nodes, profeat 70 wide, dragon 37 wide, labels planted in vector and graph); --dataset takes a .jbl (joblib) dict with
dense_adj | adj, feature, label, the vector modality and -- for the regression -- mask_label.

    python examples/train_vecmodal.py --model vec|regression [--epochs 30] [--batch 50] [--dataset x.jbl] [--save PATH]

--save PATH writes the trained model's state dict (torch.save), which examples/visualize_vecmodal.py --params reads.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kgcn_amd import cv, data_util as D, models, ops, train  # noqa: E402


def standin(kind):
    """The fixture as the .jbl dict the loaders read."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "g12_vecmodal.npz"))
    return {"dense_adj": z["ds_dense_adj"], "max_node_num": int(z["ds_max_node_num"]), "feature": z["ds_feature"],
            "profeat": z["ds_profeat"], "dragon": z["ds_dragon"], "mask_label": z["ds_mask_label"],
            "label": z["ds_label_reg"] if kind == "regression" else z["ds_label_cls"], "sizes": z["ds_sizes"]}


def fit(kind, raw, epochs=30, batch=50, lr=1e-3, seed=0, device="cuda:0", log=print):
    """-> (model, per-epoch list of dicts: training_cost, validation_cost and validation_accuracy | validation_mse)."""
    dev = torch.device(device)
    regression = kind == "regression"
    channels, _ = D.build_adjs(raw)
    feature = np.asarray(raw["feature"], np.float32)
    label = np.asarray(raw["label"], np.float32)
    G, T = label.shape
    sizes = np.asarray(raw["sizes"], np.int64) if raw.get("sizes") is not None else np.full(G, feature.shape[1], np.int64)
    ds = D.DeviceGraphDataset(channels, feature, device=dev)
    sb = ds.static_batch(batch)
    labels = sb.add_table(torch.as_tensor(label, device=dev))
    kw = {"vectors": sb.add_table(D.vector_table(raw, "dragon" if regression else "profeat", dev))}
    if regression:
        ml = np.asarray(raw["mask_label"], np.float32) if raw.get("mask_label") is not None else np.ones_like(label)
        mask = sb.add_table(torch.as_tensor(ml, device=dev))
        kw["enabled_node_nums"] = sb.add_table(torch.as_tensor(sizes.astype(np.int32), device=dev))
    else:
        mask = sb.add_table(torch.ones(G, device=dev))              # 1 for a graph, 0 for the dummy rows of a short batch
    rs = np.random.RandomState(seed)
    tr, va = cv.holdout_split(G, 0.2, rs)
    sb.load(tr[:batch])
    torch.manual_seed(seed)
    model = (models.MultimodalRegressionGCN(T) if regression else models.MultimodalVecGCN(len(channels), T)).to(dev)
    with torch.no_grad():
        model(sb.features, sb.adjacency, **kw)                      # Keras-style build
    opt = train.TFAdam(model.parameters(), lr=lr)
    step = train.GraphedTrainStep(model, opt, model.loss, sb, labels, mask, capture_assembly=True, **kw)
    history = []
    for epoch in range(epochs):
        tr = tr.copy()
        rs.shuffle(tr)
        costs = []
        for it in range(0, len(tr), batch):
            sb.stage(tr[it:it + batch])
            costs.append(step.replay()[0])                          # one replay per step; the costs stay on the device
        row = {"training_cost": float(torch.stack(costs).sum()) / len(tr)}
        vcost = verr = vcount = 0.0
        with torch.no_grad():
            for it in range(0, len(va), batch):
                sb.load(va[it:it + batch])
                out = model(sb.features, sb.adjacency, **kw)
                if regression:
                    _, cs, err, cnt = ops.masked_squared_error(out, labels, mask)
                    verr, vcount = verr + float(err.sum()), vcount + float(cnt.sum())
                else:
                    cs = model.loss(out, labels, mask)[1]
                    verr += float(((out.argmax(1) == labels.argmax(1)).float() * mask).sum())
                    vcount += float(mask.sum())
                vcost += float(cs)
        row["validation_cost"] = vcost / max(len(va), 1)
        row["validation_mse" if regression else "validation_accuracy"] = verr / vcount if vcount else float("nan")
        history.append(row)
        if log:
            log("epoch %2d  training cost %.5f  validation cost %.5f  validation %s %.4f"
                % (epoch, row["training_cost"], row["validation_cost"], "mse" if regression else "accuracy",
                   row["validation_mse" if regression else "validation_accuracy"]))
    return model, history


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("vec", "regression"), required=True)
    ap.add_argument("--epochs", type=int, default=30)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--dataset", default=None)
    ap.add_argument("--save", default=None, help="write the trained model's state dict here (torch.save)")
    a = ap.parse_args(argv)
    if a.dataset:
        import joblib
        raw = joblib.load(a.dataset)
    else:
        raw = standin(a.model)
    model, _ = fit(a.model, raw, a.epochs, a.batch, a.lr)
    if a.save:
        torch.save(model.state_dict(), a.save)
        print("state dict saved to %s" % a.save)


if __name__ == "__main__":
    main()
