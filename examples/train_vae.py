#!/usr/bin/env python3
"""kgcn-gen --config example_config/vae.json train, on the MI355X path: example_model/model_vae.py's graph VAE on the reference's
synthetic dataset (the copy kept as a test fixture: tests/golden/g1_synthetic_raw.npz = the arrays of example_jbl/synthetic.jbl),
batch 30, learning rate 1e-4, validation split 0.1 (180 / 20 graphs), TF-style Adam.  The dataset lives in HBM; every mini-batch
is assembled on the device and the whole step (forward with its Philox noise, fused reconstruction loss, backward, optimiser) is
one hipGraph replay.  Prints cost and correct_count accuracy per epoch and saves the reconstruction of the validation set (the
reference's `prediction`: sigmoid of the decoded features and adjacency) as an .npz.

    python examples/train_vae.py [epochs (100, as vae.json)] [output .npz (vae_reconstruction.npz)]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kgcn_amd import data_util as D, models, train  # noqa: E402

epochs = int(sys.argv[1]) if len(sys.argv) > 1 else 100
out_path = sys.argv[2] if len(sys.argv) > 2 else "vae_reconstruction.npz"
dev = torch.device("cuda:0")
raw = np.load(os.path.join(ROOT, "tests", "golden", "g1_synthetic_raw.npz"))
channels, _ = D.build_adjs({"dense_adj": raw["dense_adj"].astype(np.int64), "max_node_num": int(raw["max_node_num"])})
dataset = D.DeviceGraphDataset(channels, raw["feature"], device=dev)
BATCH = 30
n_valid = int(round(0.1 * dataset.num_graphs))                       # validation_data_rate 0.1
train_idx, valid_idx = np.arange(dataset.num_graphs - n_valid), np.arange(dataset.num_graphs - n_valid, dataset.num_graphs)

torch.manual_seed(0)
model = models.GraphVAE(raw["feature"].shape[2], adj_channel_num=len(channels), seed=1234).to(dev)
adj0, x0 = dataset.batch(train_idx[:BATCH], BATCH)
model(x0, adj0, graph_mask=torch.ones(BATCH, device=dev))          # creates the parameters (Keras-style lazy build)
opt = train.TFAdam(model.parameters(), lr=1e-4)
model.bind_step(opt._t_dev)                                          # noise of step t = f(seed, t), drawn on the device
batch = dataset.static_batch(BATCH)
mask = batch.add_table(torch.ones(dataset.num_graphs, device=dev))  # 1 per real graph, 0 per dummy: same assembly launch
batch.load(train_idx[:BATCH])
step = train.GraphedTrainStep(model, opt, model.loss, batch, mask, mask, capture_assembly=True, graph_mask=mask)
correct_static = model.correct_count                                 # the captured step's correct_count output


def evaluate(idx_all):
    cost, correct = 0.0, 0.0
    with torch.no_grad():
        for it in range(0, len(idx_all), BATCH):
            idx = idx_all[it:it + BATCH]
            adj, x = dataset.batch(idx, BATCH)
            m = (torch.arange(BATCH, device=dev) < len(idx)).float()
            model(x, adj, graph_mask=m)
            cost += float(model.cost_sum) * BATCH
            correct += float(model.correct_count)
    return cost / len(idx_all), correct / len(idx_all)


rng = np.random.default_rng(1234)
for epoch in range(epochs):
    rng.shuffle(train_idx)
    cost, correct = 0.0, 0.0
    for it in range(0, len(train_idx), BATCH):
        batch.stage(train_idx[it:it + BATCH])
        cs, _ = step.replay()
        cost += float(cs) * BATCH                                    # cost_sum = reduce_mean(cost) over the padded batch
        correct += float(correct_static)
    vcost, vacc = evaluate(valid_idx)
    print("epoch %3d  training cost %.5f  accuracy %.4f  validation cost %.5f  accuracy %.4f"
          % (epoch, cost / len(train_idx), correct / len(train_idx), vcost, vacc))

feats, adjs = [], []
for it in range(0, len(valid_idx), BATCH):
    idx = valid_idx[it:it + BATCH]
    adj, x = dataset.batch(idx, BATCH)
    f, a = model.reconstruct(x, adj)
    feats.append(f[:len(idx)].cpu().numpy())
    adjs.append(a[:len(idx)].cpu().numpy())
np.savez(out_path, graph_index=valid_idx, feature=np.concatenate(feats), dense_adj=np.concatenate(adjs))
print("reconstruction of %d validation graphs -> %s" % (len(valid_idx), out_path))
