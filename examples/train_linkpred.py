#!/usr/bin/env python3
"""sample_kg/network_prediction/run.sh <gcn|distmult|ip> on the MI355X path: `kgcn train` then `kgcn infer` with
config/config_<model>.json (embedding_dim 128, label_batch_size 1000, validation_data_rate 0.2, learning rate 0.001 / 0.01 /
0.001) on the BA model network of the test fixture (tests/golden/g8_kg_linkpred.npz: preprocessing_link_pred.py of a seeded
80/20 edge split).  The label list, the epoch's row permutation and the negative table live in HBM; the whole step (label batch
assembly with its Philox negatives, model, ranking loss, backward, TF-Adam) is one hipGraph replay; floor(M / 1000) steps per
epoch.  Prints the training and validation cost and accuracy (correct_count / count) per epoch; infer writes what gcn.py infer
writes: prediction_data (lp_prediction over all node pairs) and the edge result {output: H, score [M', 2]} of the test list.

    python examples/train_linkpred.py <gcn|distmult|ip> [epochs (100, as the configs)] [output directory (result_<model>)]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kgcn_amd import data_util as D, models, train  # noqa: E402

variant = sys.argv[1] if len(sys.argv) > 1 else "gcn"
epochs = int(sys.argv[2]) if len(sys.argv) > 2 else 100
out_dir = sys.argv[3] if len(sys.argv) > 3 else "result_%s" % variant
LR = {"gcn": 0.001, "distmult": 0.01, "ip": 0.001}[variant]
BATCH = 1000
dev = torch.device("cuda:0")
z = np.load(os.path.join(ROOT, "tests", "golden", "g8_kg_linkpred.npz"))
data = D.LinkPredictionData({"adj": [(z["adj_idx"], z["adj_val"], np.array([int(z["node_num"])] * 2))], "node": z["node"],
                             "node_num": z["node_num"], "label_list": z["label_list"], "test_label_list": z["test_label_list"]})
rng = np.random.RandomState(1234)
train_list, valid_list = D.split_label_list(data.label_list, 0.2, rng)          # kgcn/data_util.py:661-695
adj = data.adjacency(dev) if variant == "gcn" else None
feed = D.LinkPredFeed(train_list, batch=BATCH, adjacency=adj, device=dev)
valid_feed = D.LinkPredFeed(valid_list, adjacency=adj, device=dev)                # the whole list in one batch (label_itr None)
test_feed = D.LinkPredFeed(data.test_label_list, adjacency=adj, device=dev)

torch.manual_seed(0)
model = models.LinkPredictionNet(variant, data.num_nodes, data.num_relations, seed=1234, device=dev)
model(None, adj, feed=feed)                                                        # creates the parameters (Keras-style lazy build)
opt = train.TFAdam(model.parameters(), lr=LR)
model.bind_step(opt._t_dev)                                                        # window and negatives of step t, on the device
step = train.GraphedTrainStep(model, opt, model.loss, feed, None, None, feed=feed)
correct_static = model.correct_count                                               # the captured step's correct_count output
eval_step = torch.zeros((), dtype=torch.int64, device=dev)


def evaluate(f, epoch):
    eval_step.fill_(epoch)
    with torch.no_grad():
        model(None, adj, feed=f, seed=4321, step=eval_step)
    return float(model.cost_sum), float(model.correct_count)


for epoch in range(epochs):
    feed.shuffle(rng)                                                              # shuffle_label_list, uploaded once
    cost, correct = 0.0, 0.0
    for it in range(feed.steps_per_epoch):
        cs, _ = step.replay()
        cost += float(cs)
        correct += float(correct_static)
    vcost, vcorrect = evaluate(valid_feed, epoch)
    # kgcn/core.py: costs divided by train_data.num = 1 (one graph); accuracy = correct_count / count
    print("epoch %3d  training cost %.5f  accuracy %.4f  validation cost %.5f  accuracy %.4f"
          % (epoch, cost, correct / (feed.steps_per_epoch * BATCH), vcost, vcorrect / valid_feed.num_labels), flush=True)

tcost, tcorrect = evaluate(test_feed, epochs)
print("test cost %.5f  accuracy %.4f" % (tcost, tcorrect / test_feed.num_labels))
pred, h = model.predict(adj)
pred = pred.cpu().numpy()
tl = data.test_label_list.astype(np.int64)
if pred.ndim == 3:                                                                 # gcn.py:590-594
    score = np.stack([pred[0, tl[:, 0], tl[:, 2]], pred[0, tl[:, 3], tl[:, 5]]], 1)
else:
    score = np.stack([pred[0, tl[:, 1], tl[:, 0], tl[:, 2]], pred[0, tl[:, 4], tl[:, 3], tl[:, 5]]], 1)
os.makedirs(out_dir, exist_ok=True)
np.save(os.path.join(out_dir, "pred_data.npy"), pred)
extra = {"relation_w": model.distmult.w[0].detach().cpu().numpy()} if variant == "distmult" else {}    # for enrich_linkpred.py
np.savez(os.path.join(out_dir, "test_edge_result.npz"), output=h.detach().cpu().numpy(), score=score, **extra)
print("prediction_data %s and edge result (output %s, score %s) -> %s" % (pred.shape, tuple(h.shape), score.shape, out_dir))
