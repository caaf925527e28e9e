#!/usr/bin/env python3
"""kgcn visualize of the vector-modality models on the MI355X path: integrated gradients of

  --model vec         example_model/model_multimodal_vec.py (models.MultimodalVecGCN): node features, the channel-0 adjacency
                      values and the per-graph vector `profeat`; score = the softmax probability of the target class
  --model regression  example_model/model_multimodal_regression.py (models.MultimodalRegressionGCN): node features and the vector
                      `dragon` (the network never reads the adjacency); score = the prediction column itself

through visualization.vecmodal_integrated_gradients: the vector branch's first layer is computed once per compound and swept
over the scaled copies by the kernels of csrc/vecig.hip.  Loads parameters examples/train_vecmodal.py saved (--params, its
--save PATH), or does a short fit itself (--epochs).  Writes one {header}_{id:04d}_task_0_{assay}_{modal}_scaling.jbl per compound
(joblib, the keys kgcn/visualization.py dumps; <vector>_IG is [1, Dv]) and logs the prediction score, check score (end - start)
and sum of IG of each.

The default dataset is the synthetic stand-in of tests/golden/g12_vecmodal.npz (see examples/train_vecmodal.py); --dataset takes
a .jbl (joblib) dict with dense_adj | adj, feature, label and the vector modality.

    python examples/visualize_vecmodal.py --model vec|regression [--params FILE] [--epochs 5] [--dataset x.jbl] [--out viz_vec]
                                          [--modal all|features|adjs|profeat|dragon] [--method ig|grad_prod|grad|smooth_grad|smooth_ig]
                                          [--label-target max] [--divide-number 100] [--noise-scale 0.1] [--seed 1234]
                                          [--limit N] [--header mol] [--composed]
"""
import argparse
import importlib.util
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kgcn_amd import data_util as D, models, visualization as V  # noqa: E402


def _trainer():
    spec = importlib.util.spec_from_file_location("train_vecmodal_example", os.path.join(ROOT, "examples", "train_vecmodal.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(argv=None):
    import joblib
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("vec", "regression"), required=True)
    ap.add_argument("--modal", default="all", help="all, features, adjs (vec only) or the vector's name (profeat / dragon)")
    ap.add_argument("--method", default="ig", choices=V.IG_METHODS + V.SMOOTH_METHODS)
    ap.add_argument("--label-target", default="max")
    ap.add_argument("--divide-number", type=int, default=100)
    ap.add_argument("--noise-scale", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=1234, help="seed of the device noise of smooth_grad / smooth_ig")
    ap.add_argument("--dataset", default=None)
    ap.add_argument("--params", default=None, help="a state dict examples/train_vecmodal.py --save wrote")
    ap.add_argument("--epochs", type=int, default=5, help="epochs of the short fit when no --params are given")
    ap.add_argument("--out", default="viz_vec")
    ap.add_argument("--limit", type=int, default=None, help="visualise the first N compounds only")
    ap.add_argument("--header", default="mol")
    ap.add_argument("--composed", action="store_true", help="run the vectors through the model and autograd (fused=False)")
    a = ap.parse_args(argv)

    dev = torch.device("cuda:0")
    trainer = _trainer()
    raw = joblib.load(a.dataset) if a.dataset else trainer.standin(a.model)
    regression = a.model == "regression"
    name = "dragon" if regression else "profeat"
    channels, _ = D.build_adjs(raw)
    feature, label = np.asarray(raw["feature"], np.float32), np.asarray(raw["label"], np.float32)
    sizes = np.asarray(raw["sizes"], np.int64) if raw.get("sizes") is not None else None
    dataset = D.DeviceGraphDataset(channels, feature, device=dev)
    vectors = D.vector_table(raw, name, dev)
    if a.params:
        model = (models.MultimodalRegressionGCN(label.shape[1]) if regression else models.MultimodalVecGCN(len(channels), label.shape[1])).to(dev)
        adj, x = dataset.batch([0])
        with torch.no_grad():
            model(x, adj, vectors=vectors[:1])                       # Keras-style build, then the saved values
        model.load_state_dict(torch.load(a.params, map_location=dev))
        print("parameters loaded from %s" % a.params)
    else:
        model, hist = trainer.fit(a.model, raw, epochs=a.epochs, device=str(dev), log=None)
        print("short fit: %d epochs, training cost per graph %.5f -> %.5f" % (a.epochs, hist[0]["training_cost"], hist[-1]["training_cost"]))
    label_target = a.label_target if a.label_target in ("max", "all", "label", "correct", "uncorrect") else int(a.label_target)
    ids = list(range(dataset.num_graphs))[:a.limit]

    os.makedirs(a.out, exist_ok=True)
    torch.cuda.synchronize()
    t0 = time.time()
    results = V.vecmodal_integrated_gradients(model, None, dataset, vectors, labels=label, divide_number=a.divide_number, modal=a.modal,
                                              method=a.method, label_target=label_target, compounds=ids,
                                              fused=False if a.composed else None, noise_scale=a.noise_scale, seed=a.seed,
                                              enabled_node_nums=sizes if regression else None)
    elapsed = time.time() - t0
    files = []
    for r in results:
        path = os.path.join(a.out, V.ig_filename(a.header, r["compound_id"], r["assay"], a.modal))
        with open(path, "wb") as f:
            joblib.dump(V.dump_record(r), f)
        files.append(path)
        print("[SAVE] %s" % path)
        print("No.%d: prediction score: %.6f  check score: %.6f  sum of IG: %.6f  |difference| %.2e"
              % (r["compound_id"], r["prediction_score"], r["check_score"], r["sum_of_IG"], abs(r["check_score"] - r["sum_of_IG"])))
    print("time: %.3f s for %d dumps" % (elapsed, len(results)))
    return files


if __name__ == "__main__":
    main()
