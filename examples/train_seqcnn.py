#!/usr/bin/env python3
"""kgcn train --config config_cnn.json (sample_protein/sequence: cnn.py:SeqCNN), on the MI355X path: Embedding, three Conv1D +
MaxPooling1D layers, Conv1D(1, tanh), BatchNormalization, Dense(52), BatchNormalization, relu, Dense(label_dim) with the
class-weighted softmax cross entropy; embedding_dim 25, batch size 1, learning rate 1e-4, validation split 0.2, TF-style Adam, 20
epochs, as the config.  The sample's own sequences are downloaded by its 00get_fasta.py; by default this runs on the synthetic
stand-in kept as a test fixture (tests/golden/g9_seqcnn.npz: two classes told apart by a planted motif), and --dataset takes a
dataset.jbl written by the sample's 02make_dataset.py.  The token table lives in HBM, every mini-batch is assembled on the device
and the whole step is one hipGraph replay with the sequences as the model's forward keyword.  Prints cost and accuracy per epoch.

    python examples/train_seqcnn.py [--epochs 20] [--batch-size 1] [--learning-rate 1e-4] [--dataset dataset.jbl] [--save PATH]

--save PATH writes the trained model's state dict (torch.save), which examples/visualize_seqcnn.py --params reads.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kgcn_amd import data_util as D, models, train  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--epochs", type=int, default=20)
ap.add_argument("--batch-size", type=int, default=1)
ap.add_argument("--learning-rate", type=float, default=1e-4)
ap.add_argument("--dataset", default=None, help="dataset.jbl of 02make_dataset.py (default: the committed synthetic fixture)")
ap.add_argument("--save", default=None, help="write the trained model's state dict here (torch.save)")
args = ap.parse_args()

dev = torch.device("cuda:0")
if args.dataset:
    import joblib
    raw = joblib.load(args.dataset)
else:
    raw = np.load(os.path.join(ROOT, "tests", "golden", "g9_seqcnn.npz"))
label = np.asarray(raw["label"], np.float32)
G = label.shape[0]
tokens, S = D.sequence_table({"sequence": raw["sequence"], "sequence_symbol_num": raw["sequence_symbol_num"]}, dev)
# the sample's dataset carries a dummy 2 x 2 graph per sequence (02make_dataset.py: make_dummy_adjs); the model never reads it
channels, _ = D.build_adjs({"dense_adj": np.tile(np.eye(2, dtype=np.float32), (G, 1, 1)), "max_node_num": 2})
dataset = D.DeviceGraphDataset(channels, np.zeros((G, 2, 2), np.float32), device=dev)
BATCH = args.batch_size
order = np.random.default_rng(1234).permutation(G)                    # shuffle_data
n_valid = int(round(0.2 * G))                                         # validation_data_rate 0.2
train_idx, valid_idx = order[:G - n_valid].copy(), order[G - n_valid:]

torch.manual_seed(0)
model = models.SeqCNN(S, embedding_dim=25, label_dim=label.shape[1], class_weight=np.asarray(raw["class_weight"])).to(dev)
batch = dataset.static_batch(BATCH)
seqs = batch.add_table(tokens)                                        # int32 token rows, zeros for the dummy rows of a short batch
labels = batch.add_table(torch.as_tensor(label, device=dev))
mask = batch.add_table(torch.ones(G, device=dev))                     # 1 per real sequence, 0 per padded row
batch.load(train_idx[:BATCH])
model(batch.features, batch.adjacency, sequences=seqs)               # creates the parameters (Keras-style lazy build)
opt = train.TFAdam(model.parameters(), lr=args.learning_rate)
step = train.GraphedTrainStep(model, opt, model.loss, batch, labels, mask, capture_assembly=True, sequences=seqs)


def correct(logits, lab, m):
    return float(((logits.argmax(1) == lab.argmax(1)).float() * m).sum())


def evaluate(idx_all):
    cost, right = 0.0, 0.0
    with torch.no_grad():
        for it in range(0, len(idx_all), BATCH):
            batch.load(idx_all[it:it + BATCH])
            logits = model(batch.features, batch.adjacency, sequences=seqs)
            _, cs = model.loss(logits, labels, mask)
            cost += float(cs)
            right += correct(logits, labels, mask)
    return cost / len(idx_all), right / len(idx_all)


rng = np.random.default_rng(4321)
history = []
for epoch in range(args.epochs):
    rng.shuffle(train_idx)
    cost, right = 0.0, 0.0
    for it in range(0, len(train_idx), BATCH):
        batch.stage(train_idx[it:it + BATCH])
        cs, logits = step.replay()
        cost += float(cs)                                            # cost_sum = reduce_sum(cross entropy), unweighted
        right += correct(logits, labels, mask)
    vcost, vacc = evaluate(valid_idx)
    history.append(cost / len(train_idx))
    print("epoch %3d  training cost %.5f  accuracy %.4f  validation cost %.5f  accuracy %.4f"
          % (epoch, cost / len(train_idx), right / len(train_idx), vcost, vacc))
print("training cost %.5f -> %.5f over %d epochs" % (history[0], history[-1], args.epochs))
if args.save:
    torch.save(model.state_dict(), args.save)
    print("state dict saved to %s" % args.save)
