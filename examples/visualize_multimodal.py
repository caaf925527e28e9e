#!/usr/bin/env python3
"""kgcn visualize --config config_mm.json, on the MI355X path: integrated gradients of the multimodal model
(example_model/model_multimodal.py, models.MultimodalGCN) on the reference's example_jbl/sample.jbl (the test fixture
tests/golden/g7_sample_multimodal.npz), over the node features, the channel-0 adjacency values and the embedded protein sequence.
Loads parameters saved with torch.save(model.state_dict()) (--params), or first trains with the setup of
examples/train_multimodal.py (batch 10, TF-style Adam at 0.3, --epochs).  Writes one
{header}_{id:04d}_task_0_{assay}_{modal}_scaling.jbl per compound (joblib, the keys kgcn/visualization.py dumps) and logs the
prediction score, check score (end - start) and sum of IG of each compound and the accuracy over the visualised ones.

--method smooth_grad / smooth_ig average --divide-number noisy samples (N(0, --noise-scale) on the targeted inputs, drawn on
the device from --seed); file names and dump keys are the same for every method.

    python examples/visualize_multimodal.py [--params FILE] [--epochs 5] [--outdir viz_mm] [--modal all]
                                            [--method ig|grad_prod|grad|smooth_grad|smooth_ig] [--noise-scale 0.1] [--seed 1234]
                                            [--label-target max] [--divide-number 100] [--header mol]
"""
import argparse
import os
import sys
import time

import joblib
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kgcn_amd import data_util as D, models, train, visualization as V  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--params", default=None, help="state_dict of a MultimodalGCN (torch.save(model.state_dict()))")
ap.add_argument("--epochs", type=int, default=5, help="training epochs when no --params are given")
ap.add_argument("--outdir", default="viz_mm")
ap.add_argument("--modal", default="all", choices=("all",) + V.IG_MODALS)
ap.add_argument("--method", default="ig", choices=V.IG_METHODS + V.SMOOTH_METHODS)
ap.add_argument("--noise-scale", type=float, default=0.1, help="standard deviation of the noise of the smooth methods")
ap.add_argument("--seed", type=int, default=1234, help="seed of the noise of the smooth methods")
ap.add_argument("--label-target", default="max")
ap.add_argument("--divide-number", type=int, default=100)
ap.add_argument("--header", default="mol")
args = ap.parse_args()

dev = torch.device("cuda:0")
raw = np.load(os.path.join(ROOT, "tests", "golden", "g7_sample_multimodal.npz"))
channels, _ = D.build_adjs({"dense_adj": raw["dense_adj"], "max_node_num": int(raw["max_node_num"])})
tokens, S = D.sequence_table({"sequence": raw["sequence"], "sequence_symbol_num": raw["sequence_symbol_num"]}, dev)
dataset = D.DeviceGraphDataset(channels, raw["feature"], device=dev)
torch.manual_seed(0)
model = models.MultimodalGCN(S, embedding_dim=4, adj_channel_num=len(channels), label_dim=raw["label"].shape[1]).to(dev)
BATCH = 10
batch = dataset.static_batch(BATCH)
seqs = batch.add_table(tokens)
labels = batch.add_table(torch.as_tensor(raw["label"], dtype=torch.float32, device=dev))
mask = batch.add_table(torch.ones(dataset.num_graphs, device=dev))
n_valid = int(round(0.3 * dataset.num_graphs))
train_idx = np.arange(dataset.num_graphs - n_valid)
batch.load(train_idx[:BATCH])
model(batch.features, batch.adjacency, sequences=seqs)               # creates the parameters (Keras-style lazy build)
if args.params:
    model.load_state_dict(torch.load(args.params, map_location=dev))
    print("parameters loaded from %s" % args.params)
else:
    opt = train.TFAdam(model.parameters(), lr=0.3)
    step = train.GraphedTrainStep(model, opt, models.MultimodalGCN.loss, batch, labels, mask, capture_assembly=True, sequences=seqs)
    rng = np.random.default_rng(1234)
    for epoch in range(args.epochs):
        rng.shuffle(train_idx)
        cost = 0.0
        for it in range(0, len(train_idx), BATCH):
            batch.stage(train_idx[it:it + BATCH])
            cs, _ = step.replay()
            cost += float(cs)
        print("epoch %3d  training cost %.5f" % (epoch, cost / len(train_idx)))

os.makedirs(args.outdir, exist_ok=True)
t0 = time.time()
results = V.multimodal_integrated_gradients(model, None, dataset, tokens, labels=raw["label"], divide_number=args.divide_number,
                                            modal=args.modal, method=args.method, label_target=args.label_target,
                                            noise_scale=args.noise_scale, seed=args.seed)
elapsed = time.time() - t0
correct = 0
for r in results:
    name = V.ig_filename(args.header, r["compound_id"], r["assay"], args.modal)
    with open(os.path.join(args.outdir, name), "wb") as f:
        joblib.dump(V.dump_record(r), f)
    print("[SAVE] %s" % os.path.join(args.outdir, name))
    print("No.%d: prediction score: %.6f  check score: %.6f  sum of IG: %.6f  |difference| %.2e"
          % (r["compound_id"], r["prediction_score"], r["check_score"], r["sum_of_IG"], abs(r["check_score"] - r["sum_of_IG"])))
    if r["true_label"] is not None:
        with torch.no_grad():
            adj, x = dataset.batch([r["compound_id"]])
            pred_label = int(model(x, adj, sequences=tokens[r["compound_id"]:r["compound_id"] + 1]).argmax(1))
        correct += int(pred_label == r["true_label"])
print("time: %.3f s for %d compounds" % (elapsed, len(results)))
if results:
    print("accuracy(visualized_data) = %.4f" % (correct / len(results)))
