#!/usr/bin/env python3
"""kgcn train --config example_config/multimodal.json, on the MI355X path: example_model/model_multimodal.py (graph branch +
protein-sequence branch) on the reference's example_jbl/sample.jbl (the copy kept as a test fixture:
tests/golden/g7_sample_multimodal.npz), batch 10, learning rate 0.3, validation split 0.3, TF-style Adam, 5 epochs.  The dataset,
its token table included, lives in HBM; every mini-batch is assembled on the device (a short batch gets zero token rows for its
dummy graphs, kgcn/feed.py:178-181) and the whole step is one hipGraph replay.  Prints cost and accuracy per epoch.

    python examples/train_multimodal.py [epochs (5, as multimodal.json)]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kgcn_amd import data_util as D, models, train  # noqa: E402

epochs = int(sys.argv[1]) if len(sys.argv) > 1 else 5
dev = torch.device("cuda:0")
raw = np.load(os.path.join(ROOT, "tests", "golden", "g7_sample_multimodal.npz"))
channels, _ = D.build_adjs({"dense_adj": raw["dense_adj"], "max_node_num": int(raw["max_node_num"])})
tokens, S = D.sequence_table({"sequence": raw["sequence"], "sequence_symbol_num": raw["sequence_symbol_num"]}, dev)
dataset = D.DeviceGraphDataset(channels, raw["feature"], device=dev)
BATCH = 10
n_valid = int(round(0.3 * dataset.num_graphs))                       # validation_data_rate 0.3
train_idx, valid_idx = np.arange(dataset.num_graphs - n_valid), np.arange(dataset.num_graphs - n_valid, dataset.num_graphs)

torch.manual_seed(0)
model = models.MultimodalGCN(S, embedding_dim=4, adj_channel_num=len(channels), label_dim=raw["label"].shape[1]).to(dev)
batch = dataset.static_batch(BATCH)
seqs = batch.add_table(tokens)                                        # int32 token rows, zeros for the dummy graphs
labels = batch.add_table(torch.as_tensor(raw["label"], dtype=torch.float32, device=dev))
mask = batch.add_table(torch.ones(dataset.num_graphs, device=dev))   # 1 per real graph, 0 per dummy
batch.load(train_idx[:BATCH])
model(batch.features, batch.adjacency, sequences=seqs)               # creates the parameters (Keras-style lazy build)
opt = train.TFAdam(model.parameters(), lr=0.3)
step = train.GraphedTrainStep(model, opt, models.MultimodalGCN.loss, batch, labels, mask, capture_assembly=True, sequences=seqs)


def correct(logits, lab, m):
    return float(((logits.argmax(1) == lab.argmax(1)).float() * m).sum())


def evaluate(idx_all):
    cost, right = 0.0, 0.0
    with torch.no_grad():
        for it in range(0, len(idx_all), BATCH):
            batch.load(idx_all[it:it + BATCH])
            logits = model(batch.features, batch.adjacency, sequences=seqs)
            _, cs = models.MultimodalGCN.loss(logits, labels, mask)
            cost += float(cs)
            right += correct(logits, labels, mask)
    return cost / len(idx_all), right / len(idx_all)


rng = np.random.default_rng(1234)
history = []
for epoch in range(epochs):
    rng.shuffle(train_idx)
    cost, right = 0.0, 0.0
    for it in range(0, len(train_idx), BATCH):
        batch.stage(train_idx[it:it + BATCH])
        cs, logits = step.replay()
        cost += float(cs)                                            # cost_sum = reduce_sum(mask * cross entropy)
        right += correct(logits, labels, mask)
    vcost, vacc = evaluate(valid_idx)
    history.append(cost / len(train_idx))
    print("epoch %3d  training cost %.5f  accuracy %.4f  validation cost %.5f  accuracy %.4f"
          % (epoch, cost / len(train_idx), right / len(train_idx), vcost, vacc))
print("training cost %.5f -> %.5f over %d epochs" % (history[0], history[-1], epochs))
